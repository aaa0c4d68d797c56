// spectator_events.hip -- the GgrsEvent queue of the spectator engine's sessions (spectator.hip,
// spectator_ingest.hip, spectator_poll.hip): SpectatorSession::handle_event
// (src/sessions/p2p_spectator_session.rs:199-239) over the net_events row the endpoint poll wrote, kept
// per session on the device, and SpectatorSession::events() for every session in one call.  A
// spectator's queue is the first part of the P2P session's step (events_device.h, kSession = false): its
// one host endpoint's NetworkResumed, NetworkInterrupted and Disconnected, every push and every handled
// Input followed by the trim to MAX_EVENT_QUEUE_SIZE, so a queue never holds more than 100 events.
// GGRS_NET_DISCONNECTED stands for both causes of a Disconnected here, as in spectator_poll.hip.
#include <hip/hip_runtime.h>

#include "common.h"
#include "events_device.h"
#include "spectator_engine.h"

using namespace ggrs;

namespace {

__global__ __launch_bounds__(kEvBlock) void spectator_events_kernel(EvCollect p) { ev_collect_walk<false>(p); }

int ev_need(ggrs_spectator_engine_t* e, const char* what) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->evq.on) return set_error(GGRS_E_STATE, "%s needs ggrs_spectator_set_event_queue", what);
  return GGRS_OK;
}

}  // namespace

namespace ggrs {

int spectator_events_free(ggrs_spectator_engine* e) {
  e->evq.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_spectator_set_event_queue(ggrs_spectator_engine_t* e, int32_t capacity) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->calls != 0 || e->next_arrival_call != 0)
    return set_error(GGRS_E_STATE, "the event queue is part of the engine's configuration (set before the first arrival and "
                     "call)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->evq.configure((size_t)e->cfg.num_sessions, capacity, e->stream);
}

int ggrs_spectator_collect_events(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, const uint8_t* handled_inputs,
                                  const uint8_t* net_events, int32_t on_device) {
  if (int rc = ev_need(e, "collecting events")) return rc;
  EventQueueHost& q = e->evq;
  if (int rc = q.check_calls(first_call, n)) return rc;
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  // host-sourced calls: [handled_inputs][net_events] staged
  const uint8_t *d_handled = handled_inputs, *d_net = net_events;
  if (!on_device) {
    if (int rc = grow_staging(&q.staging, &q.staging_bytes, 2 * rows)) return rc;
    if (handled_inputs) {
      HIP_TRY(hipMemcpyAsync(q.staging, handled_inputs, rows, hipMemcpyHostToDevice, e->stream));
      d_handled = q.staging;
    }
    if (net_events) {
      HIP_TRY(hipMemcpyAsync(q.staging + rows, net_events, rows, hipMemcpyHostToDevice, e->stream));
      d_net = q.staging + rows;
    }
  }
  if (int rc = e->timer.before(e->stream)) return rc;
  const EvCollect p{(int64_t)S,
                    first_call,
                    n,
                    q.capacity,
                    0,
                    0u,
                    e->poll.on ? e->poll.timeout - e->poll.notify : 0,
                    0,
                    nullptr,
                    nullptr,
                    d_handled,
                    d_net,
                    nullptr,
                    nullptr,
                    reinterpret_cast<uint4*>(q.ring),
                    q.st,
                    nullptr,
                    q.stage_count};
  spectator_events_kernel<<<grid_of((int64_t)S, kEvBlock), kEvBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));  // (the caller's arrays are free again)
  q.next = first_call + n;
  return GGRS_OK;
}

int ggrs_spectator_drain_events(ggrs_spectator_engine_t* e, int32_t max_records, int32_t* session,
                                ggrs_event_record_t* records, int32_t* n_read, int32_t* n_left, int32_t on_device) {
  if (int rc = ev_need(e, "draining events")) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  return ev_drain(e->evq, max_records, session, records, n_read, n_left, on_device, e->stream);
}

int ggrs_spectator_read_event_queue_state(ggrs_spectator_engine_t* e, int32_t* length, int32_t* dropped, int32_t* status,
                                          int32_t* closed_call, ggrs_event_record_t* queue) {
  if (int rc = ev_need(e, "the event queues' state")) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->evq.read(length, dropped, status, closed_call, queue, e->stream);
}

}  // extern "C"
