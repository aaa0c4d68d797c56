// p2p_time_sync.hip -- time sync of the any-network P2P engine (p2p_sched.hip, p2p_ingest.hip,
// p2p_emit.hip): every session's frames_ahead and GgrsEvent::WaitRecommendation on the device, the one
// statement of P2PSession::advance_frame the other units leave out.  This is check_wait_recommendation
// (src/sessions/p2p_session.rs:357, :804-817) with max_frame_advantage (:786-802), the endpoint's TimeSync
// (src/time_sync.rs:25-39), UdpProtocol::update_local_frame_advantage (src/network/protocol.rs:260-269,
// called from poll_remote_clients, p2p_session.rs:442-447), on_quality_report (protocol.rs:649-653),
// on_quality_reply, and the window push inside send_input (:433-437), for one endpoint per session
// holding all of its remote players (packet emit's simplification).
//
// Per session: round_trip_time, remote_frame_advantage, local_frame_advantage and
// next_recommended_sleep 0, the two windows of FRAME_WINDOW_SIZE = 30 entries zeros, the endpoint open.
// Call c, after it ran, in the reference's order:
//   1. a stopped session (emit_ll holds kEmitStopped from its stopping call on) takes no step:
//      frames_ahead 0, skip_frames 0, local_advantage the last value;
//   2. intake, while the endpoint is open: rtt_ms[c] >= 0 sets round_trip_time, remote_advantage[c] !=
//      GGRS_TIME_SYNC_KEEP sets remote_frame_advantage, clamped to i16 as send_quality_report clamps what
//      it sends (protocol.rs:504-508);
//   3. update_local_frame_advantage(cur), while the endpoint is open and last_recv != NULL_FRAME:
//      local_frame_advantage = last_recv + ((round_trip_time / 2) * fps) / 1000 - cur.  cur is
//      SyncLayer::current_frame at the start of the call: add_local_input queues frame cur + input_delay
//      and drops a repeat (input_queue.rs:170-186), so cur = emit_ll[c] - input_delay whether the call's
//      input was accepted or not; last_recv is the feed's ack row, else the running maximum of the
//      arrival rows, as the emits derive it;
//   4. an Event::Disconnected bit of a remote player closes the endpoint from here on
//      (disconnect_player_at_frame, p2p_session.rs:618-655; poll_remote_clients updates the advantage
//      before it handles the poll's events);
//   5. frames_ahead = average_frame_advantage() while the endpoint is open, else 0 -- from the windows
//      before this call's push, time_sync.rs:30-39 literally: (f32)local_sum / 30.0f, (f32)remote_sum /
//      30.0f, ((remote_avg - local_avg) / 2.0f) truncated.  cur > next_recommended_sleep && frames_ahead
//      >= MIN_RECOMMENDATION (3): next_recommended_sleep = cur + RECOMMENDATION_INTERVAL (60),
//      skip_frames = frames_ahead; else skip_frames = 0;
//   6. the push inside send_input, while the endpoint is open and the call's add_local_input was
//      accepted (emit_ll rose): local[(cur + input_delay) % 30] = local_frame_advantage, remote[...] =
//      remote_frame_advantage;
//   7. local_advantage[c] = local_frame_advantage after the call.
// Stated divergence from the reference: round_trip_time above 1 << 20 ms is clamped there (the
// reference overflows only beyond i32; the clamp keeps ping * fps inside i32 for fps <= 1000).
//
// The two f32 divisions are correctly rounded (build.py: no fast-math) and stay two divisions in the
// reference's order: in exact integers (remote_sum - local_sum) / 60 differs from them, sums of -400
// and -220 give 2 here and 3 exactly.
//
// One thread per session, one wave per block; the launch's calls are walked in order because the
// windows carry from call to call.  The windows live in HBM, [2][30][S]; their sums are held in
// registers, rebuilt from the windows at the launch's start (60 coalesced loads: no second copy of the
// truth between launches).  kLds (the default): the block's windows sit in LDS for the launch (15 KB)
// and go back at its end; else a push reads and writes its slot in HBM, a dependent round trip on about
// every call, which measured 1.5x the time.  A group of calls' words is loaded before its first use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "emit_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int32_t kKeep = GGRS_TIME_SYNC_KEEP;
constexpr int32_t kMaxRtt = 1 << 20;
constexpr int32_t kMinRecommendation = 3;      // MIN_RECOMMENDATION (p2p_session.rs)
constexpr int32_t kRecommendationInterval = 60;  // RECOMMENDATION_INTERVAL
constexpr int kTsBlock = kEmitBlock;
constexpr int kTsGroup = kEmitGroup;

struct TsParams {
  int64_t S;
  int32_t cap, c0, n;
  int32_t pkt, delay, fps;
  uint32_t rmask;              // the remote players' event bits
  const int32_t* ll;           // [cap][S] the local players' last queued frame after the call, or kEmitStopped
  const int32_t* arrive;       // [cap][S] (the packet feed off)
  const int32_t* pkt_ack;      // [cap][S] (the packet feed on)
  const uint8_t* events;       // [cap][S]
  const int32_t* rtt;          // [n][S] or null
  const int32_t* radv;         // [n][S] or null
  int32_t* win;                // [2][kTsWindow][S]
  int32_t* st;                 // [kTsFields][S]
  int32_t* o_local;            // [n][S]
  int32_t* o_ahead;            // [n][S]
  int32_t* o_skip;             // [n][S]
};

template <bool kLds>
__global__ __launch_bounds__(kTsBlock) void p2p_time_sync_kernel(TsParams p) {
  __shared__ int32_t s_win[kLds ? 2 * kTsWindow * kTsBlock : 1];
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int64_t s0 = (int64_t)blockIdx.x * kTsBlock;
  const int nb = (int)min((int64_t)kTsBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;  // idle lanes shadow the block's first session, never store
  const int32_t cap = p.cap;
  auto fld = [&](int f) -> int32_t& { return p.st[(int64_t)f * S + s]; };
  int32_t rtt = fld(kTsRtt), remote = fld(kTsRemote), local = fld(kTsLocal), next_sleep = fld(kTsNextSleep);
  int32_t closed = fld(kTsClosedCall), ll_prev = fld(kTsLlPrev), recv = fld(kTsRecv);
  // the windows' sums (and, kLds, the windows: column t is this thread's own, no barrier needed)
  int32_t lsum = 0, rsum = 0;
#pragma unroll
  for (int i = 0; i < kTsWindow; i++) {
    const int32_t l = p.win[(int64_t)i * S + s], r = p.win[(int64_t)(kTsWindow + i) * S + s];
    lsum += l;
    rsum += r;
    if (kLds) {
      s_win[i * kTsBlock + t] = l;
      s_win[(kTsWindow + i) * kTsBlock + t] = r;
    }
  }

  for (int32_t k0 = 0; k0 < p.n; k0 += kTsGroup) {
    const int gn = min(kTsGroup, p.n - k0);
    // the group's per-call words, all loads in flight together (a short group repeats its last call)
    int32_t ll8[kTsGroup], rcv8[kTsGroup], rtt8[kTsGroup], adv8[kTsGroup];
    uint32_t ev8[kTsGroup];
#pragma unroll
    for (int g = 0; g < kTsGroup; g++) {
      const int32_t k = k0 + min(g, gn - 1);
      const int64_t o = (int64_t)((p.c0 + k) % cap) * S + s, in_i = (int64_t)k * S + s;
      ll8[g] = p.ll[o];
      ev8[g] = p.events[o];
      rcv8[g] = p.pkt ? p.pkt_ack[o] : p.arrive[o];
      rtt8[g] = p.rtt ? p.rtt[in_i] : -1;
      adv8[g] = p.radv ? p.radv[in_i] : kKeep;
    }
    for (int g = 0; g < gn; g++) {
      const int32_t c = p.c0 + k0 + g;
      // this call's words: the front of the batch, which shifts down a call per iteration (indexing it by
      // g would put it in scratch memory)
      const int32_t ll = ll8[0], rcv = rcv8[0], rtt_in = rtt8[0], adv_in = adv8[0];
      const uint32_t ev = ev8[0] & p.rmask;
#pragma unroll
      for (int j = 0; j < kTsGroup - 1; j++) {
        ll8[j] = ll8[j + 1];
        rcv8[j] = rcv8[j + 1];
        rtt8[j] = rtt8[j + 1];
        adv8[j] = adv8[j + 1];
        ev8[j] = ev8[j + 1];
      }
      int32_t ahead = 0, skip = 0;
      if (ll != kEmitStopped) {  // 1.
        const int32_t cur = ll - p.delay;
        recv = p.pkt ? rcv : max(recv, rcv);
        bool open = closed < 0;
        if (open) {
          // 2. on_quality_reply, on_quality_report (protocol.rs:649-653)
          if (rtt_in >= 0) rtt = min(rtt_in, kMaxRtt);
          if (adv_in != kKeep) remote = min(max(adv_in, -32768), 32767);
          // 3. update_local_frame_advantage (:260-269)
          if (recv != kNull) local = recv + ((rtt / 2) * p.fps) / 1000 - cur;
          // 4. disconnect_player_at_frame
          if (ev) {
            closed = c;
            open = false;
          }
        }
        if (open) {
          // 5. average_frame_advantage (time_sync.rs:30-39)
          const float local_avg = (float)lsum / 30.0f;
          const float remote_avg = (float)rsum / 30.0f;
          ahead = (int32_t)((remote_avg - local_avg) / 2.0f);
        }
        if (cur > next_sleep && ahead >= kMinRecommendation) {
          next_sleep = cur + kRecommendationInterval;
          skip = ahead;
        }
        // 6. send_input's time_sync_layer.advance_frame (:433-437)
        if (open && ll != ll_prev) {
          const int slot = (int)((uint32_t)ll % (uint32_t)kTsWindow);
          int32_t old_l, old_r;
          if (kLds) {
            old_l = s_win[slot * kTsBlock + t];
            old_r = s_win[(kTsWindow + slot) * kTsBlock + t];
            s_win[slot * kTsBlock + t] = local;
            s_win[(kTsWindow + slot) * kTsBlock + t] = remote;
          } else {
            int32_t* wl = p.win + (int64_t)slot * S + s;
            int32_t* wr = p.win + (int64_t)(kTsWindow + slot) * S + s;
            old_l = *wl;
            old_r = *wr;
            if (live) {
              *wl = local;
              *wr = remote;
            }
          }
          lsum += local - old_l;
          rsum += remote - old_r;
        }
        ll_prev = ll;
      }
      if (live) {
        const int64_t o = (int64_t)(k0 + g) * S + s;
        p.o_local[o] = local;  // 7.
        p.o_ahead[o] = ahead;
        p.o_skip[o] = skip;
      }
    }
  }
  if (live) {
    fld(kTsRtt) = rtt;
    fld(kTsRemote) = remote;
    fld(kTsLocal) = local;
    fld(kTsNextSleep) = next_sleep;
    fld(kTsClosedCall) = closed;
    fld(kTsLlPrev) = ll_prev;
    fld(kTsRecv) = recv;
    if (kLds) {
#pragma unroll
      for (int i = 0; i < 2 * kTsWindow; i++) p.win[(int64_t)i * S + s] = s_win[i * kTsBlock + t];
    }
  }
}

// GGRS_TIME_SYNC_LDS=0 touches a push's slot in HBM instead of holding the block's windows in LDS for
// the launch (for the comparison; default 1, which measured 0.78 against 1.15 us per call of 65,536
// sessions, profiles/time_sync_rate.json)
bool ts_lds_from_env() {
  const char* v = std::getenv("GGRS_TIME_SYNC_LDS");
  return !(v && v[0] == '0');
}

}  // namespace

namespace ggrs {

int p2p_time_sync_free(ggrs_p2p_engine* e) {
  if (e->tsync_win) (void)hipFree(e->tsync_win);
  if (e->tsync_st) (void)hipFree(e->tsync_st);
  e->tsync_win = nullptr;
  e->tsync_st = nullptr;
  e->tsync.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_time_sync(ggrs_p2p_engine_t* e, int32_t fps) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "time sync is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "time sync needs ggrs_p2p_set_arrival_schedule(e, 1)");
  if (e->peer_reports) return set_error(GGRS_E_STATE, "time sync with peers' disconnect reports is not supported");
  const uint32_t all = (1u << e->cfg.num_players) - 1u, lm = (uint32_t)e->cfg.local_mask & all;
  if (!lm || lm == all) return set_error(GGRS_E_INVALID, "time sync needs a local and a remote player");
  if (fps < 1 || fps > 1000) return set_error(GGRS_E_INVALID, "fps must be in 1..1000, got %d", fps);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  if (int rc = p2p_emit_ll_alloc(e)) return rc;
  if (!e->tsync_st) {
    HIP_TRY(hipMalloc(&e->tsync_win, sizeof(int32_t) * 2 * (size_t)kTsWindow * S));
    HIP_TRY(hipMalloc(&e->tsync_st, sizeof(int32_t) * (size_t)kTsFields * S));
  }
  HIP_TRY(hipMemsetAsync(e->tsync_win, 0, sizeof(int32_t) * 2 * (size_t)kTsWindow * S, e->stream));
  // every session: no round trip measured, no advantage either way, no recommendation made, the endpoint open
  constexpr uint32_t kZero = 1u << kTsRtt | 1u << kTsRemote | 1u << kTsLocal | 1u << kTsNextSleep;
  if (int rc = emit_fill(e->tsync_st, S, kTsFields, kZero, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->tsync.configure(0, 0);
  e->tsync_fps = fps;
  return GGRS_OK;
}

int ggrs_p2p_time_sync(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* rtt_ms,
                       const int32_t* remote_advantage, int32_t* local_advantage, int32_t* frames_ahead,
                       int32_t* skip_frames, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->tsync.on) return set_error(GGRS_E_STATE, "time sync needs ggrs_p2p_set_time_sync");
  PacketEmitState& ts = e->tsync;
  const int32_t oldest_held = std::max(e->next_input_frame, e->next_arrival_call) - e->cap;
  if (int rc = ts.check_order(first_call, n, e->current_frame, oldest_held, e->cap,
                              !local_advantage || !frames_ahead || !skip_frames, "time sync runs"))
    return rc;
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  // host-sourced calls: [rtt][remote_advantage][local_advantage][frames_ahead][skip_frames] staged (stream
  // order keeps an earlier launch's use of the buffer ahead of the copies)
  const int32_t *d_rtt = rtt_ms, *d_radv = remote_advantage;
  int32_t *d_local = local_advantage, *d_ahead = frames_ahead, *d_skip = skip_frames;
  if (!on_device) {
    if (int rc = grow_staging(&ts.staging, &ts.staging_bytes, 5 * sizeof(int32_t) * rows)) return rc;
    int32_t* base = reinterpret_cast<int32_t*>(ts.staging);
    d_local = base + 2 * rows;
    d_ahead = base + 3 * rows;
    d_skip = base + 4 * rows;
    if (rtt_ms) {
      HIP_TRY(hipMemcpyAsync(base, rtt_ms, 4 * rows, hipMemcpyHostToDevice, e->stream));
      d_rtt = base;
    }
    if (remote_advantage) {
      HIP_TRY(hipMemcpyAsync(base + rows, remote_advantage, 4 * rows, hipMemcpyHostToDevice, e->stream));
      d_radv = base + rows;
    }
  }
  if (int rc = e->timer.before(e->stream)) return rc;
  const uint32_t rmask = ~(uint32_t)e->cfg.local_mask & ((1u << e->cfg.num_players) - 1u);
  const TsParams p{(int64_t)S, e->cap, first_call, n, e->pkt, e->cfg.input_delay, e->tsync_fps, rmask, e->emit_ll,
                   e->arrive, e->feed.ack, e->events, d_rtt, d_radv, e->tsync_win, e->tsync_st, d_local, d_ahead, d_skip};
  const int64_t grid = grid_of((int64_t)S, kTsBlock);
  if (ts_lds_from_env())
    p2p_time_sync_kernel<true><<<grid, kTsBlock, 0, e->stream>>>(p);
  else
    p2p_time_sync_kernel<false><<<grid, kTsBlock, 0, e->stream>>>(p);
  HIP_TRY(hipGetLastError());
  e->timer.count();
  if (!on_device) {
    HIP_TRY(hipMemcpyAsync(local_advantage, d_local, 4 * rows, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(frames_ahead, d_ahead, 4 * rows, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(skip_frames, d_skip, 4 * rows, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  ts.next = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_read_time_sync_state(ggrs_p2p_engine_t* e, int32_t* local_advantage, int32_t* remote_advantage,
                                  int32_t* rtt_ms, int32_t* next_recommended_sleep, int32_t* closed_call,
                                  int32_t* windows) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->tsync.on)
    return set_error(GGRS_E_STATE, "the time-sync state exists with ggrs_p2p_set_time_sync only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  auto rd = [&](int32_t* dst, int f) { return read_field(dst, e->tsync_st, f, S, e->stream); };
  HIP_TRY(rd(local_advantage, kTsLocal));
  HIP_TRY(rd(remote_advantage, kTsRemote));
  HIP_TRY(rd(rtt_ms, kTsRtt));
  HIP_TRY(rd(next_recommended_sleep, kTsNextSleep));
  HIP_TRY(rd(closed_call, kTsClosedCall));
  if (windows)
    HIP_TRY(hipMemcpyAsync(windows, e->tsync_win, sizeof(int32_t) * 2 * (size_t)kTsWindow * S, hipMemcpyDeviceToHost,
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

}  // extern "C"
