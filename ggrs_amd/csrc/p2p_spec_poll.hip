// p2p_spec_poll.hip -- the poll of the any-network P2P engine's spectator endpoints (p2p_spec_emit.hip
// is their send side): P2PSession::poll_remote_clients' spectator loop (src/sessions/p2p_session.rs:458-464)
// with handle_event (:866-878), disconnect_player (:506-509) and disconnect_player_at_frame's spectator
// branch (:645-652), over UdpProtocol::poll (src/network/protocol.rs:329-376) and the clock bookkeeping
// of handle_message (:534-551), per call, on the device, for the K endpoints of every session.  It
// decides what the host's 200 ms timers decided for them: that the retry is due (resend, spectator
// emit's input), that a quality report is due (send_report), that a spectator went quiet
// (NetworkInterrupted) or came back (NetworkResumed), and that it is gone -- it timed out, the host
// disconnected it (close_in), or its pending inputs overflowed in spectator emit -- after which the
// endpoint goes from Running over Disconnected to Shutdown and spectator emit stops streaming to it.
//
// The step is poll_device.h's, as PollOwner::kSessionSpectator.  A spectator sends no Input: an Input
// bit in kinds counts as a message and nothing else (the reference would decode it and then hit the
// assert! of p2p_session.rs:882 -- a stated divergence), so there is no send_ack output, and nothing but
// the retry itself ever resets running_last_input_recv: the retry recurs every time more than 200 ms
// have passed.  Neither close_in nor the overflow sets disconnect_event_sent; the reference's paths do
// not.  The overflow is the Event::Disconnected send_input queues (protocol.rs:443-445), which the
// reference handles at the next poll: it is read from spectator emit's endpoint status as of the launch,
// so it lands at the reference's call when each call's emit precedes the next call's poll (the live
// loop), and at the next launch's first call when the polls run further ahead.  A spectator's timeout
// does not enter the game: no events row is written, the session and its other endpoints are untouched.
//
// One thread per endpoint over [K][S] rows, the same coalesced rows with K * S endpoints; the launch loop
// is poll_device.h's poll_walk.
#include <hip/hip_runtime.h>

#include "common.h"
#include "p2p_engine.h"
#include "poll_device.h"

using namespace ggrs;

namespace {

struct SpecEpPollParams {
  PollWalk w;
  const uint8_t* kinds;        // [n][K][S] or null
  const uint8_t* close_in;     // [n][K][S] or null
  const int32_t* emit_status;  // [K][S] spectator emit's endpoint status (kSpecEpStatus)
};

struct SpectatorIo {
  const SpecEpPollParams& p;
  uint32_t over = 0;  // spectator emit closed the endpoint with GGRS_EMIT_DISCONNECTED before this launch
  __device__ inline void begin(int64_t e) { over = p.emit_status[e] == GGRS_EMIT_DISCONNECTED ? (kPollExt | kPollExtEvent) : 0u; }
  __device__ inline void load(int32_t k, int32_t, int64_t e, uint32_t& kd, uint32_t& ev, int32_t& st) const {
    const int64_t i = (int64_t)k * p.w.E + e;
    kd = p.kinds ? p.kinds[i] : 0u;
    ev = p.close_in ? p.close_in[i] : 0u;
    st = 0;
  }
  __device__ inline bool decoded(uint32_t, int32_t) const { return false; }
  __device__ inline uint32_t ext(uint32_t ev) const { return (ev != 0 ? kPollExt : 0u) | over; }
  __device__ inline void raised(int32_t, int64_t, uint32_t) const {}  // (a spectator's timeout does not enter the game)
};

__global__ __launch_bounds__(kPollBlock) void p2p_spec_poll_kernel(SpecEpPollParams p) {
  poll_walk<PollOwner::kSessionSpectator>(p.w, SpectatorIo{p});
}

}  // namespace

namespace ggrs {

int p2p_spec_poll_free(ggrs_p2p_engine* e) {
  e->spoll.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_spectator_poll(ggrs_p2p_engine_t* e, uint64_t disconnect_timeout_ms, uint64_t disconnect_notify_start_ms,
                                uint64_t start_ms) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "the spectator endpoint poll is part of the session's configuration (set before the first "
                     "call)");
  if (!e->sched || !e->spec.on) return set_error(GGRS_E_STATE, "the spectator endpoint poll needs ggrs_p2p_set_spectator_emit");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->spoll.configure((size_t)e->spec_k * (size_t)e->cfg.num_sessions, disconnect_timeout_ms, disconnect_notify_start_ms,
                            start_ms, e->stream);
}

int ggrs_p2p_poll_spectator_endpoints(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const uint64_t* now_ms,
                                      const uint8_t* kinds, const uint8_t* close_in, uint8_t* resend, uint8_t* send_report,
                                      uint8_t* net_events, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->spec.on || !e->spoll.on)
    return set_error(GGRS_E_STATE, "polling the spectator endpoints needs ggrs_p2p_set_spectator_poll");
  if (int rc = e->spoll.check_calls(first_call, n, now_ms, on_device)) return rc;
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const PollHost::Io host{now_ms, {kinds, close_in}, {resend, nullptr, send_report, net_events}};
  PollHost::Io dev;
  if (int rc = e->spoll.begin(host, (size_t)n, on_device, e->stream, &dev)) return rc;
  if (int rc = e->timer.before(e->stream)) return rc;
  const int64_t E = (int64_t)e->spoll.E;
  const SpecEpPollParams p{{E, first_call, n, e->spoll.timeout, e->spoll.notify, dev.now, e->spoll.clock_in(),
                            e->spoll.clock_out(), e->spoll.times, e->spoll.st, dev.out[0], nullptr, dev.out[2], dev.out[3]},
                           dev.in[0], dev.in[1], e->spec_ep + (int64_t)kSpecEpStatus * E};
  p2p_spec_poll_kernel<<<grid_of(E, kPollBlock), kPollBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return e->spoll.end(host, dev, first_call, (size_t)n, on_device, e->stream);
}

int ggrs_p2p_read_spectator_endpoint_state(ggrs_p2p_engine_t* e, int32_t* state, uint64_t* last_recv_ms,
                                           uint64_t* last_input_recv_ms, uint64_t* last_report_ms, uint64_t* shutdown_ms,
                                           int32_t* flags, int32_t* closed_call) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->spec.on || !e->spoll.on)
    return set_error(GGRS_E_STATE, "the spectator endpoints' state exists with ggrs_p2p_set_spectator_poll only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->spoll.read(state, last_recv_ms, last_input_recv_ms, last_report_ms, shutdown_ms, flags, closed_call, e->stream);
}

}  // extern "C"
