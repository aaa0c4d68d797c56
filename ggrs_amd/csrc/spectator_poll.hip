// spectator_poll.hip -- the endpoint poll of the spectator engine (spectator.hip, spectator_ingest.hip):
// SpectatorSession::poll_remote_clients (src/sessions/p2p_spectator_session.rs:133-156) with handle_event
// (:199-239) over the host endpoint's UdpProtocol::poll (src/network/protocol.rs:329-376), the clock
// bookkeeping of handle_message (:534-551) and on_input's disconnect_requested, running_last_input_recv
// and send_input_ack (:569-574, :608, :634), per call, on the device.  It decides what a spectator's
// host-side timers decided: that an Input was decoded and is acknowledged (send_ack), that a quality
// report is due (send_report), that the host went quiet (NetworkInterrupted) or came back
// (NetworkResumed), and that the host is gone (GgrsEvent::Disconnected: it asked for the disconnect, or
// it timed out -- GGRS_NET_DISCONNECTED stands for both, the engine has no events row in which the
// requested one could be seen).
//
// Where this unit differs from the P2P one (p2p_poll.hip): the reference's spectator never calls
// host.disconnect() -- handle_event only forwards the event -- so the endpoint stays Running for good,
// its timers and the interrupted / resumed pair go on after the one Disconnected, and
// GGRS_NET_SHUTDOWN never appears.  The step (poll_device.h) has that as PollOwner::kSpectatorHost.  The
// retry timer has no output, because a spectator has nothing pending; it is kept so that
// running_last_input_recv equals the reference's.  The poll changes nothing in the sessions: a
// spectator whose host is gone waits, as the reference's does.
//
// One thread per session; the launch loop is poll_device.h's poll_walk.  This unit's own part: kinds and
// events are the caller's [n][S] arrays, and with the packet feed on the feed's status row of the call
// says whether its Input was decoded.
#include <hip/hip_runtime.h>

#include "common.h"
#include "poll_device.h"
#include "spectator_engine.h"

using namespace ggrs;

namespace {

struct SpecPollParams {
  PollWalk w;
  int32_t cap, pkt;
  const uint8_t* kinds;    // [n][S] or null
  const uint8_t* events;   // [n][S] or null
  const int32_t* status;   // [cap][S] the feed's status row (the packet feed on)
};

struct HostIo {
  const SpecPollParams& p;
  __device__ inline void begin(int64_t) {}
  __device__ inline void load(int32_t k, int32_t c, int64_t s, uint32_t& kd, uint32_t& ev, int32_t& st) const {
    const int64_t i = (int64_t)k * p.w.E + s;
    kd = p.kinds ? p.kinds[i] : 0u;
    ev = p.events ? p.events[i] : 0u;
    st = p.pkt ? p.status[(int64_t)(c % p.cap) * p.w.E + s] : 0;
  }
  __device__ inline bool decoded(uint32_t kd, int32_t st) const { return (kd & (1u << GGRS_WIRE_INPUT)) != 0 && st >= 0; }
  __device__ inline uint32_t ext(uint32_t ev) const { return ev != 0 ? kPollExt : 0u; }
  __device__ inline void raised(int32_t, int64_t, uint32_t) const {}  // (the session only forwards the event)
};

__global__ __launch_bounds__(kPollBlock) void spectator_poll_kernel(SpecPollParams p) {
  poll_walk<PollOwner::kSpectatorHost>(p.w, HostIo{p});
}

}  // namespace

namespace ggrs {

int spectator_poll_free(ggrs_spectator_engine* e) {
  e->poll.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_spectator_set_endpoint_poll(ggrs_spectator_engine_t* e, uint64_t disconnect_timeout_ms,
                                     uint64_t disconnect_notify_start_ms, uint64_t start_ms) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->calls != 0 || e->next_arrival_call != 0)
    return set_error(GGRS_E_STATE, "the endpoint poll is part of the engine's configuration (set before the first arrival "
                     "and call)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->poll.configure((size_t)e->cfg.num_sessions, disconnect_timeout_ms, disconnect_notify_start_ms, start_ms, e->stream);
}

int ggrs_spectator_poll_endpoints(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, const uint64_t* now_ms,
                                  const uint8_t* kinds, const uint8_t* events, uint8_t* send_ack, uint8_t* send_report,
                                  uint8_t* net_events, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->poll.on) return set_error(GGRS_E_STATE, "polling the endpoints needs ggrs_spectator_set_endpoint_poll");
  if (int rc = e->poll.check_calls(first_call, n, now_ms, on_device)) return rc;
  if (n == 0) return GGRS_OK;
  if (e->pkt) {
    if ((int64_t)first_call + n > e->next_arrival_call)
      return set_error(GGRS_E_INVALID, "a call is polled after its packets were received (received up to call %d, polls need "
                       "up to %d)", e->next_arrival_call - 1, first_call + n - 1);
    if (first_call < e->next_arrival_call - e->cap)
      return set_error(GGRS_E_INVALID, "call %d's packet status is no longer held (the last %d calls' are)", first_call, e->cap);
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  const PollHost::Io host{now_ms, {kinds, events}, {nullptr, send_ack, send_report, net_events}};
  PollHost::Io dev;
  if (int rc = e->poll.begin(host, (size_t)n, on_device, e->stream, &dev)) return rc;
  if (int rc = e->timer.before(e->stream)) return rc;
  const SpecPollParams p{{(int64_t)e->cfg.num_sessions, first_call, n, e->poll.timeout, e->poll.notify, dev.now,
                          e->poll.clock_in(), e->poll.clock_out(), e->poll.times, e->poll.st, nullptr, dev.out[1], dev.out[2],
                          dev.out[3]},
                         e->cap, e->pkt, dev.in[0], dev.in[1], e->feed.status};
  spectator_poll_kernel<<<grid_of(p.w.E, kPollBlock), kPollBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return e->poll.end(host, dev, first_call, (size_t)n, on_device, e->stream);
}

int ggrs_spectator_read_endpoint_state(ggrs_spectator_engine_t* e, uint64_t* last_recv_ms, uint64_t* last_input_recv_ms,
                                       uint64_t* last_report_ms, int32_t* flags, int32_t* disconnected_call) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->poll.on) return set_error(GGRS_E_STATE, "the endpoints' state exists with ggrs_spectator_set_endpoint_poll only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->poll.read(nullptr, last_recv_ms, last_input_recv_ms, last_report_ms, nullptr, flags, disconnected_call, e->stream);
}

}  // extern "C"
