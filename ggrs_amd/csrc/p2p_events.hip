// p2p_events.hip -- the GgrsEvent queue of the any-network P2P engine's sessions (p2p_sched.hip and the
// units around it): P2PSession::event_queue (src/sessions/p2p_session.rs:149) as advance_frame fills
// it (:265-357) -- handle_event's pushes and its trim to MAX_EVENT_QUEUE_SIZE (:846-902) over the rows
// the endpoint poll and the spectator endpoint poll wrote, the DesyncDetected records of the checksum
// comparison (:904-937) and time sync's WaitRecommendation (:804-817) -- kept per session on the
// device, and P2PSession::events() (:573-576) for every session in one call: a drain into one dense
// list.  The step, the collect loop and the drain are events_device.h's, shared with
// spectator_events.hip; this unit's own part is the P2P session's rows, the desync record list (the
// caller's arrays, or the comparison's own list on the device) and the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "events_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

__global__ __launch_bounds__(kEvBlock) void p2p_events_kernel(EvCollect p) { ev_collect_walk<true>(p); }

int ev_need(ggrs_p2p_engine_t* e, const char* what) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->evq.on) return set_error(GGRS_E_STATE, "%s needs ggrs_p2p_set_event_queue", what);
  return GGRS_OK;
}

}  // namespace

namespace ggrs {

int p2p_events_free(ggrs_p2p_engine* e) {
  e->evq.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_event_queue(ggrs_p2p_engine_t* e, int32_t capacity) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "the event queue is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "the event queue needs ggrs_p2p_set_arrival_schedule(e, 1)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->evq.configure((size_t)e->cfg.num_sessions, capacity, e->stream);
}

int ggrs_p2p_collect_events(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const uint8_t* events, const uint8_t* disc_req,
                            const uint8_t* handled_inputs, const uint8_t* net_events, const uint8_t* spec_net_events,
                            const int32_t* skip_frames, int32_t n_desync, const int32_t* ds_call, const int32_t* ds_session,
                            const int32_t* ds_frame, const uint16_t* ds_local, const uint16_t* ds_remote, int32_t on_device) {
  if (int rc = ev_need(e, "collecting events")) return rc;
  EventQueueHost& q = e->evq;
  if (int rc = q.check_calls(first_call, n)) return rc;
  const bool own_list = n_desync == -1;
  if (n_desync < -1) return set_error(GGRS_E_INVALID, "n_desync must be >= 0, or -1 for the engine's own list");
  if (own_list && (ds_call || ds_session || ds_frame || ds_local || ds_remote))
    return set_error(GGRS_E_INVALID, "n_desync == -1 takes the engine's own list: the record arrays must be NULL");
  if (n_desync > 0 && (!ds_call || !ds_session || !ds_frame || !ds_local || !ds_remote))
    return set_error(GGRS_E_INVALID, "null argument");
  if (own_list) {
    if (!e->dcmp.on) return set_error(GGRS_E_STATE, "the engine's own desync list needs ggrs_p2p_set_desync_compare");
    if (n > 0 && e->dcmp.next < first_call + n)
      return set_error(GGRS_E_STATE, "call %d has not been compared (ggrs_p2p_compare_reports ran through call %d, collecting "
                       "needs it through call %d)", e->dcmp.next, e->dcmp.next - 1, first_call + n - 1);
  }
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, K = (size_t)e->spec_k, rows = (size_t)n * S;

  // the desync records: the engine's own list from the first record no collection has taken, or the
  // caller's arrays
  int64_t list_first = 0, list_end = n_desync;
  const int32_t *d_call = ds_call, *d_session = ds_session, *d_frame = ds_frame, *d_words = nullptr;
  const uint16_t *d_local = ds_local, *d_remote = ds_remote;
  if (own_list) {
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->dcmp_count, sizeof(total), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t me = (size_t)e->dcmp_max_events;
    list_first = q.list_from;
    list_end = (int64_t)std::min<unsigned long long>(total, (unsigned long long)me);
    d_call = e->dcmp_events;
    d_session = e->dcmp_events + me;
    d_frame = e->dcmp_events + 2 * me;
    d_words = e->dcmp_events + 3 * me;
    d_local = d_remote = nullptr;
  }
  const bool any_records = list_end > list_first;
  if (any_records)
    if (int rc = q.need_stage()) return rc;

  // host-sourced calls: [skip_frames][ds_call][ds_session][ds_frame][ds_local][ds_remote][the five byte
  // rows] staged (stream order keeps an earlier launch's use of the buffer ahead of the copies)
  const uint8_t* d_rows[5] = {events, disc_req, handled_inputs, net_events, spec_net_events};
  const int32_t* d_skip = skip_frames;
  if (!on_device) {
    const size_t nd = own_list ? 0 : (size_t)n_desync, ndp = (nd + 1) & ~(size_t)1;  // (the u16 arrays keep dword alignment)
    const size_t row_bytes[5] = {rows, rows, rows, rows, rows * K};
    if (int rc = grow_staging(&q.staging, &q.staging_bytes, 4 * rows + 12 * nd + 4 * ndp + 4 * rows + rows * K)) return rc;
    uint8_t* at = q.staging;
    hipError_t err = hipSuccess;
    auto up = [&](const void* src, size_t bytes, size_t reserve) -> const uint8_t* {
      uint8_t* dst = at;
      at += reserve;
      if (!src || !bytes) return nullptr;
      if (err == hipSuccess) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream);
      return dst;
    };
    const uint8_t* got[11];
    got[0] = up(skip_frames, 4 * rows, 4 * rows);
    got[1] = up(own_list ? nullptr : ds_call, 4 * nd, 4 * nd);
    got[2] = up(own_list ? nullptr : ds_session, 4 * nd, 4 * nd);
    got[3] = up(own_list ? nullptr : ds_frame, 4 * nd, 4 * nd);
    got[4] = up(own_list ? nullptr : ds_local, 2 * nd, 2 * ndp);
    got[5] = up(own_list ? nullptr : ds_remote, 2 * nd, 2 * ndp);
    for (int i = 0; i < 5; i++) got[6 + i] = up(d_rows[i], row_bytes[i], row_bytes[i]);
    HIP_TRY(err);
    d_skip = reinterpret_cast<const int32_t*>(got[0]);
    if (!own_list) {
      d_call = reinterpret_cast<const int32_t*>(got[1]);
      d_session = reinterpret_cast<const int32_t*>(got[2]);
      d_frame = reinterpret_cast<const int32_t*>(got[3]);
      d_local = reinterpret_cast<const uint16_t*>(got[4]);
      d_remote = reinterpret_cast<const uint16_t*>(got[5]);
    }
    for (int i = 0; i < 5; i++) d_rows[i] = got[6 + i];
  }
  if (int rc = e->timer.before(e->stream)) return rc;
  if (any_records)
    if (int rc = ev_bucket(q, first_call, n, list_first, list_end, d_call, d_session, d_frame, d_local, d_remote, d_words,
                           e->stream))
      return rc;
  const uint32_t rmask = ~(uint32_t)e->cfg.local_mask & ((1u << e->cfg.num_players) - 1u);
  const EvCollect p{(int64_t)S,
                    first_call,
                    n,
                    q.capacity,
                    (int32_t)K,
                    rmask,
                    e->endp_on ? e->endp_timeout - e->endp_notify : 0,
                    e->spoll.on ? e->spoll.timeout - e->spoll.notify : 0,
                    d_rows[0],
                    d_rows[1],
                    d_rows[2],
                    d_rows[3],
                    K ? d_rows[4] : nullptr,
                    d_skip,
                    reinterpret_cast<uint4*>(q.ring),
                    q.st,
                    any_records ? q.stage : nullptr,
                    q.stage_count};
  p2p_events_kernel<<<grid_of((int64_t)S, kEvBlock), kEvBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));  // (the caller's arrays are free again)
  // the comparison has run exactly through these calls: every record of the list is taken
  if (own_list && e->dcmp.next == first_call + n) q.list_from = list_end;
  q.next = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_drain_events(ggrs_p2p_engine_t* e, int32_t max_records, int32_t* session, ggrs_event_record_t* records,
                          int32_t* n_read, int32_t* n_left, int32_t on_device) {
  if (int rc = ev_need(e, "draining events")) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  return ev_drain(e->evq, max_records, session, records, n_read, n_left, on_device, e->stream);
}

int ggrs_p2p_read_event_queue_state(ggrs_p2p_engine_t* e, int32_t* length, int32_t* dropped, int32_t* status,
                                    int32_t* closed_call, ggrs_event_record_t* queue) {
  if (int rc = ev_need(e, "the event queues' state")) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->evq.read(length, dropped, status, closed_call, queue, e->stream);
}

}  // extern "C"
