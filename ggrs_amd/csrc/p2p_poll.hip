// p2p_poll.hip -- the endpoint poll of the any-network P2P engine (p2p_sched.hip, p2p_ingest.hip,
// p2p_emit.hip, p2p_time_sync.hip, p2p_desync.hip): every session's UdpProtocol::poll
// (src/network/protocol.rs:329-376) with the clock bookkeeping of handle_message (:534-551), on the
// device, for one endpoint per session holding all of its remote players (packet emit's
// simplification).  It decides what the host's 200 ms timers decided: that a retry is due (resend),
// that an Input was decoded and is acknowledged (send_ack), that a quality report is due
// (send_report), that the link went silent (NetworkInterrupted) or came back (NetworkResumed), and
// that the peer timed out: Event::Disconnected, whose remote players' bits it ORs into the events row
// of the call, where the scheduled kernels, the emits and time sync read them -- the timed-out player
// is disconnected by call c itself (disconnect_player_at_frame, p2p_session.rs:618-655) and no other
// unit's code changes.  The step itself is poll_device.h's; it states why no keep_alive row exists.
//
// Call c's poll runs after call c's arrivals were added (or its packets received) and before the
// call runs; ggrs_p2p_advance_frames refuses a call that was not polled (p2p_sched.hip).
// Stated divergences: one clock per poll stands for the reference's several Instant::now() reads; a
// remote bit given to an endpoint that is already Disconnected changes nothing (the reference cannot
// raise a second Event::Disconnected); after Shutdown send_all_messages drops the queue (:401-407),
// here the host drops what the other units still produce, by the state.
//
// One thread per session; the launch loop is poll_device.h's poll_walk, shared with the two spectator
// units.  This unit's own part: the call's events byte is read from and, by the lanes whose timeout
// fired, written to the engine's events row, each lane its own byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "emit_device.h"
#include "p2p_engine.h"
#include "poll_device.h"

using namespace ggrs;

namespace {

static_assert(kPollBlock == kEmitBlock && kPollGroup == kEmitGroup, "the poll walks the emits' block and group");

struct PollParams {
  PollWalk w;
  int32_t cap, pkt;
  uint32_t rmask;              // the remote players' event bits
  const uint8_t* kinds;        // [n][S] or null
  const int32_t* status;       // [cap][S] the feed's status row (the packet feed on)
  uint8_t* events;             // [cap][S]
};

struct RemoteIo {
  const PollParams& p;
  __device__ inline void begin(int64_t) {}
  __device__ inline void load(int32_t k, int32_t c, int64_t s, uint32_t& kd, uint32_t& ev, int32_t& st) const {
    const int64_t o = (int64_t)(c % p.cap) * p.w.E + s;
    kd = p.kinds ? p.kinds[(int64_t)k * p.w.E + s] : 0u;
    ev = p.events[o];
    st = p.pkt ? p.status[o] : 0;
  }
  __device__ inline bool decoded(uint32_t kd, int32_t st) const { return (kd & (1u << GGRS_WIRE_INPUT)) != 0 && st >= 0; }
  __device__ inline uint32_t ext(uint32_t ev) const { return (ev & p.rmask) != 0 ? kPollExt : 0u; }
  // the timeout's Event::Disconnected: the call itself disconnects the remote players
  __device__ inline void raised(int32_t c, int64_t s, uint32_t ev) const {
    p.events[(int64_t)(c % p.cap) * p.w.E + s] = (uint8_t)(ev | p.rmask);
  }
};

__global__ __launch_bounds__(kPollBlock) void p2p_poll_kernel(PollParams p) {
  poll_walk<PollOwner::kSessionRemote>(p.w, RemoteIo{p});
}

__global__ void poll_fill_kernel(uint64_t* a, int64_t n, uint64_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

}  // namespace

namespace ggrs {

int p2p_poll_free(ggrs_p2p_engine* e) {
  if (e->endp_times) (void)hipFree(e->endp_times);
  if (e->endp_st) (void)hipFree(e->endp_st);
  if (e->endp_clock) (void)hipFree(e->endp_clock);
  if (e->endp_staging) (void)hipFree(e->endp_staging);
  e->endp_times = nullptr;
  e->endp_st = nullptr;
  e->endp_clock = nullptr;
  e->endp_staging = nullptr;
  e->endp_staging_bytes = 0;
  e->endp_on = 0;
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_endpoint_poll(ggrs_p2p_engine_t* e, uint64_t disconnect_timeout_ms, uint64_t disconnect_notify_start_ms,
                               uint64_t start_ms) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "the endpoint poll is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "the endpoint poll needs ggrs_p2p_set_arrival_schedule(e, 1)");
  const uint32_t all = (1u << e->cfg.num_players) - 1u, lm = (uint32_t)e->cfg.local_mask & all;
  if (!lm || lm == all) return set_error(GGRS_E_INVALID, "the endpoint poll needs a local and a remote player");
  if (disconnect_notify_start_ms > disconnect_timeout_ms)
    return set_error(GGRS_E_INVALID, "disconnect_notify_start (%llu ms) must not exceed disconnect_timeout (%llu ms)",
                     (unsigned long long)disconnect_notify_start_ms, (unsigned long long)disconnect_timeout_ms);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  // (each buffer on its own: one that failed to allocate is the only one a later call allocates)
  if (!e->endp_times) HIP_TRY(hipMalloc(&e->endp_times, sizeof(uint64_t) * (size_t)kPollTimes * S));
  if (!e->endp_st) HIP_TRY(hipMalloc(&e->endp_st, sizeof(int32_t) * (size_t)kPollFields * S));
  if (!e->endp_clock) HIP_TRY(hipMalloc(&e->endp_clock, sizeof(uint64_t) * 2));
  // every Instant of UdpProtocol::new (:219-220, :252) is start_ms, and so is shutdown_timeout (:227);
  // Running, neither flag set, never closed
  const int64_t cells = (int64_t)kPollTimes * (int64_t)S;
  poll_fill_kernel<<<grid_of(cells, 256), 256, 0, e->stream>>>(e->endp_times, cells, start_ms);
  HIP_TRY(hipGetLastError());
  poll_fill_kernel<<<1, 64, 0, e->stream>>>(e->endp_clock, 2, start_ms);
  HIP_TRY(hipGetLastError());
  if (int rc = emit_fill(e->endp_st, S, kPollFields, 1u << kPollWord, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->endp_on = 1;
  e->endp_next = 0;
  e->endp_timeout = disconnect_timeout_ms;
  e->endp_notify = disconnect_notify_start_ms;
  e->endp_host_clock = start_ms;
  e->endp_launches = 0;
  return GGRS_OK;
}

int ggrs_p2p_poll_endpoints(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const uint64_t* now_ms,
                            const uint8_t* kinds, uint8_t* resend, uint8_t* send_ack, uint8_t* send_report,
                            uint8_t* net_events, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->endp_on) return set_error(GGRS_E_STATE, "polling the endpoints needs ggrs_p2p_set_endpoint_poll");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->endp_next)
    return set_error(GGRS_E_INVALID, "endpoints are polled in call order, each call once (expected call %d, got %d)",
                     e->endp_next, first_call);
  if (n == 0) return GGRS_OK;
  if (!now_ms) return set_error(GGRS_E_INVALID, "null argument");
  if (first_call < e->current_frame)
    return set_error(GGRS_E_INVALID, "call %d already ran (a call is polled before it runs; %d calls run)", first_call,
                     e->current_frame);
  if ((int64_t)first_call + n > e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "a call is polled after its arrivals were added (added up to call %d, polls need up to %d)",
                     e->next_arrival_call - 1, first_call + n - 1);
  if (!on_device) {
    uint64_t last = e->endp_host_clock;
    for (int32_t k = 0; k < n; k++) {
      if (now_ms[k] < last)
        return set_error(GGRS_E_INVALID, "now_ms must not decrease (call %d: %llu after %llu)", first_call + k,
                         (unsigned long long)now_ms[k], (unsigned long long)last);
      last = now_ms[k];
    }
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  // host-sourced calls: [now_ms][kinds][resend][send_ack][send_report][net_events] staged (stream order
  // keeps an earlier launch's use of the buffer ahead of the copies)
  const uint64_t* d_now = now_ms;
  const uint8_t* d_kinds = kinds;
  uint8_t* d_out[4] = {resend, send_ack, send_report, net_events};
  uint8_t* const h_out[4] = {resend, send_ack, send_report, net_events};
  if (!on_device) {
    const size_t now_bytes = sizeof(uint64_t) * (size_t)n;
    if (int rc = grow_staging(&e->endp_staging, &e->endp_staging_bytes, now_bytes + 5 * rows)) return rc;
    uint8_t* base = e->endp_staging + now_bytes;
    HIP_TRY(hipMemcpyAsync(e->endp_staging, now_ms, now_bytes, hipMemcpyHostToDevice, e->stream));
    d_now = reinterpret_cast<const uint64_t*>(e->endp_staging);
    if (kinds) {
      HIP_TRY(hipMemcpyAsync(base, kinds, rows, hipMemcpyHostToDevice, e->stream));
      d_kinds = base;
    }
    for (int i = 0; i < 4; i++)
      if (h_out[i]) d_out[i] = base + (size_t)(i + 1) * rows;
  }
  if (int rc = e->timer.before(e->stream)) return rc;
  const uint32_t rmask = ~(uint32_t)e->cfg.local_mask & ((1u << e->cfg.num_players) - 1u);
  const int in = e->endp_launches & 1;
  const PollParams p{{(int64_t)S, first_call, n, e->endp_timeout, e->endp_notify, d_now, e->endp_clock + in,
                      e->endp_clock + (in ^ 1), e->endp_times, e->endp_st, d_out[0], d_out[1], d_out[2], d_out[3]},
                     e->cap, e->pkt, rmask, d_kinds, e->feed.status, e->events};
  p2p_poll_kernel<<<grid_of((int64_t)S, kPollBlock), kPollBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  e->endp_launches++;
  if (!on_device) {
    for (int i = 0; i < 4; i++)
      if (h_out[i]) HIP_TRY(hipMemcpyAsync(h_out[i], d_out[i], rows, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (the host's now_ms and kinds were read by then, too)
    e->endp_host_clock = now_ms[n - 1];
  }
  e->endp_next = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_read_endpoint_state(ggrs_p2p_engine_t* e, int32_t* state, uint64_t* last_recv_ms, uint64_t* last_input_recv_ms,
                                 uint64_t* last_report_ms, uint64_t* shutdown_ms, int32_t* flags, int32_t* closed_call) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->endp_on)
    return set_error(GGRS_E_STATE, "the endpoints' state exists with ggrs_p2p_set_endpoint_poll only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  auto rt = [&](uint64_t* dst, int f) {
    return dst ? hipMemcpyAsync(dst, e->endp_times + (size_t)f * S, sizeof(uint64_t) * S, hipMemcpyDeviceToHost, e->stream)
               : hipSuccess;
  };
  HIP_TRY(rt(last_recv_ms, kPollLastRecv));
  HIP_TRY(rt(last_input_recv_ms, kPollLastInputRecv));
  HIP_TRY(rt(last_report_ms, kPollLastReport));
  HIP_TRY(rt(shutdown_ms, kPollShutdown));
  HIP_TRY(read_field(closed_call, e->endp_st, kPollClosedCall, S, e->stream));
  std::vector<int32_t> word;
  if (state || flags) {
    word.resize(S);
    HIP_TRY(read_field(word.data(), e->endp_st, kPollWord, S, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t s = 0; s < word.size(); s++) {
    if (state) state[s] = word[s] >> kPollStateShift;
    if (flags) flags[s] = word[s] & ((1 << kPollStateShift) - 1);
  }
  return GGRS_OK;
}

}  // extern "C"
