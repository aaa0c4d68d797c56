// p2p_spec_emit.hip -- the any-network P2P engine's send side towards its sessions' spectators:
// P2PSession::send_confirmed_inputs_to_spectators (src/sessions/p2p_session.rs:716-745) with
// SyncLayer::confirmed_inputs (sync_layer.rs:296-310), and per spectator endpoint
// UdpProtocol::send_input (src/network/protocol.rs:421-448), send_pending_output (:450-487),
// pop_pending_output (:378-391) and the retry of poll (:333-337).  K endpoints per session (1..4).
//
// One pending input is P bytes, every player's confirmed byte of one frame in ascending player order.
// Per session next_spectator_frame = 0; per endpoint last_acked = (NULL_FRAME, zeros), pending empty,
// the stream open.  Call c, in the reference's order:
//   1. ack_in[c][k] pops endpoint k's pending inputs with frame <= it; last_acked is the last popped;
//   2. every frame f in [next_spectator_frame, confirmed] is pushed to every open endpoint, confirmed
//      being the call's confirmed_frame() (p2p_session.rs:542-553): the minimum over connected
//      players of the local players' last queued frame before this call's add_local_input and the
//      remote players' last received frame.  Player k's byte is zero when disconnected[k] &&
//      last_frame[k] < f under the connect status after the call's poll (blank_input), else its
//      confirmed input of frame f; next_spectator_frame = confirmed + 1;
//   3. more than max_pending_inputs pending closes that endpoint (GGRS_EMIT_DISCONNECTED);
//   4. an endpoint emits when the call pushed a frame, or resend[c][k] is set and something is
//      pending: start_frame = its first pending frame, bytes = compression::encode(last_acked,
//      pending...);
//   5. notes[c] = the call's peer_connect_status as a GGRS_SPECTATOR_NOTE word, rotating over the
//      disconnected players by call index;
//   6. a stopped session (emit_ll holds kEmitStopped from its stopping call on) takes no step;
//   7. a frame to push that reads its input row (a remote byte that is not blank) whose row slot holds
//      another frame by now (row_tag) closes the session's endpoints with GGRS_EMIT_ROW_LOST; the
//      call pushes nothing.
// Stated divergences from the reference: the reference queues one message per pushed frame, each a
// superset of the one before, and this emits the last (all a receiver taking the newest of its poll
// needs); the overflow's Event::Disconnected (:443-445) is applied at once, the overflowing call
// emitting nothing for that endpoint; with several disconnected players a spectator learns of each
// at most P - 1 delivered packets late.
//
// What the call was taken under is restated here rather than stored by the scheduled kernels: without
// peers' disconnect reports (refused together with spectator emit) confirmed_frame and the connect
// status are a function of emit_ll of the previous call, the arrival rows and the events, all of
// which packet emit already reads.  So the scheduled kernels store nothing more than for packet emit.
//
// One thread per session, one wave per block; the launch's calls are walked in order.  The confirmed
// inputs live once per session in an HBM ring [Q][S], one dword per frame, slot frame & (Q - 1): the
// local bytes enter at the call that queued their frame, the remote bytes and the blanking when the
// frame is confirmed.  The K endpoints share it: endpoint k's pending inputs are the frames
// (last_acked_k, next_spectator_frame), so an endpoint is its last_acked and its status, held in
// registers for the launch.  A call's words are loaded one call ahead of its step.  Each endpoint's
// delta and runs are streamed into an LDS packet row -- or, where an earlier endpoint of the call has
// the same last_acked and so the same packet, that endpoint's row is copied; the rows of up to 8
// calls' (call, endpoint) pairs are then written out with coalesced dword stores (emit_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "codec_device.h"
#include "common.h"
#include "emit_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kSpecMaxK = 4;  // spectator endpoints per session, at most

struct SpecParams {
  int64_t S;
  int32_t cap, c0, n, G, K;
  int32_t maxpend, stride, Pp, pkt;
  int32_t dedup;               // endpoints of a call with equal last_acked: encode once, copy the row
  uint32_t qmask;              // Q - 1
  uint32_t lmask;              // the local players
  const uint8_t* inputs;       // [cap][S] row words
  const int32_t* row_tag;      // [cap] the frame each row slot holds
  const int32_t* ll;           // [cap][S] the local players' last queued frame after the call, or kEmitStopped
  const int32_t* arrive;       // [cap][S] (the packet feed off)
  const int32_t* pkt_ack;      // [cap][S] (the packet feed on)
  const uint8_t* events;       // [cap][S]
  const int32_t* ack_in;       // [n][K][S] or null
  const uint8_t* resend;       // [n][K][S] or null
  uint32_t* ring;              // [Q][S]
  int32_t* st;                 // [kSpecFields][S]
  int32_t* ep;                 // [kSpecEpFields][K][S]
  const int32_t* poll_closed;  // [K][S] the spectator endpoint poll's closed_call (kPoll)
  int32_t* o_start;            // [n][K][S]
  int32_t* o_len;              // [n][K][S]
  int32_t* o_notes;            // [n][S]
  uint8_t* o_packets;          // [n][K][S][stride]
};

// kPoll: the engine polls its spectator endpoints (p2p_spec_poll.hip).  An endpoint the poll closed at a
// call <= c pushes and emits nothing from call c on, a retry included: its status becomes
// GGRS_EMIT_CLOSED and its closing call the poll's (send_input's early return and the is_running()
// check, protocol.rs:426, p2p_session.rs:736).  The session and its other endpoints are untouched.
template <int P, bool kPoll>
__global__ __launch_bounds__(kEmitBlock) void p2p_spec_emit_kernel(SpecParams p) {
  // [G][kEmitBlock][pitch] the packet rows of a group of (call, endpoint) pairs, then their lengths
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_maxdw;
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int pitch = odd_dword_pitch(p.stride);
  const int64_t s0 = (int64_t)blockIdx.x * kEmitBlock;
  const int nb = (int)min((int64_t)kEmitBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;  // idle lanes take no step and never store
  const int32_t cap = p.cap, K = p.K;
  constexpr uint32_t kAll = P == 4 ? 0xffffffffu : (1u << (8 * P)) - 1u;
  uint32_t lbytes = 0;
#pragma unroll
  for (int j = 0; j < P; j++)
    if ((p.lmask >> j) & 1u) lbytes |= 0xffu << (8 * j);
  const uint32_t rmask = ~p.lmask & ((1u << P) - 1u);
#define l_len (reinterpret_cast<int32_t*>(smem + (size_t)p.G * kEmitBlock * pitch))
  auto fld = [&](int f) -> int32_t& { return p.st[(int64_t)f * S + s]; };
  auto row_word = [&](int64_t o) -> uint32_t {  // every player's byte of a row
    const uint8_t* w = p.inputs + o * p.Pp;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < P; j++) v |= (uint32_t)w[j] << (8 * j);
    return v;
  };
  int32_t next = fld(kSpecNext), ll_prev = fld(kSpecLlPrev), recv = fld(kSpecRecv), lost_call = fld(kSpecLostCall);
  uint32_t disc = (uint32_t)fld(kSpecDisc);
  int32_t lf[P];
#pragma unroll
  for (int j = 0; j < P; j++) lf[j] = fld(kSpecLf0 + j);
  // the call's own words, from its session step (the pair with endpoint 0) to its last endpoint
  int32_t next_old = next, pushed = 0;
  bool stopped = false;
  // the endpoints' words, and where in the group each endpoint's packet of the current call is
  int32_t e_la[kSpecMaxK], e_pend[kSpecMaxK], e_status[kSpecMaxK], e_closed[kSpecMaxK];
  uint32_t e_lab[kSpecMaxK];
  int32_t sent_slot[kSpecMaxK], sent_len[kSpecMaxK];
  int32_t e_pc[kSpecMaxK];  // (kPoll) the poll's closing call
  auto epf = [&](int f, int j) -> int32_t& { return p.ep[((int64_t)f * K + j) * S + s]; };
#pragma unroll
  for (int j = 0; j < kSpecMaxK; j++) {
    const int jj = j < K ? j : 0;
    e_la[j] = epf(kSpecEpLaFrame, jj);
    e_lab[j] = (uint32_t)epf(kSpecEpLaBytes, jj);
    e_pend[j] = epf(kSpecEpPending, jj);
    e_status[j] = epf(kSpecEpStatus, jj);
    e_closed[j] = epf(kSpecEpClosedCall, jj);
    e_pc[j] = -1;
    if constexpr (kPoll) e_pc[j] = p.poll_closed[(int64_t)jj * S + s];
    sent_slot[j] = -1;
    sent_len[j] = 0;
  }
  int32_t i = 0, k = 0;  // the pair in hand: call c0 + i, endpoint k
  // a call's words, loaded one call ahead of its step
  int32_t n_ll = kNull, n_rcv = kNull;
  uint32_t n_ev = 0, n_word = 0;
  auto load_call = [&](int32_t ii) {
    const int64_t o = (int64_t)((p.c0 + ii) % cap) * S + s;
    n_ll = p.ll[o];
    n_rcv = p.pkt ? p.pkt_ack[o] : p.arrive[o];
    n_ev = p.events[o];
    n_word = row_word(o);
  };
  load_call(0);
  const int32_t pairs = p.n * K;
  int32_t n_ack = kNull;
  uint32_t n_rs = 0;
  auto load_pair = [&](int32_t qq) {
    const int64_t in_i = (int64_t)qq * S + s;
    n_ack = p.ack_in ? p.ack_in[in_i] : kNull;
    n_rs = p.resend ? p.resend[in_i] : 0u;
  };
  load_pair(0);

  for (int32_t q0 = 0; q0 < pairs; q0 += p.G) {
    const int gn = min(p.G, pairs - q0);
    __syncthreads();  // (the previous group's rows are written out)
    if (t == 0) s_maxdw = 0;
    __syncthreads();
    int need = 0;
#pragma unroll
    for (int j = 0; j < kSpecMaxK; j++) sent_slot[j] = -1;  // (the previous group's rows are gone)
    for (int g = 0; g < gn; g++) {
      const int32_t q = q0 + g;  // = i * K + k
      const int32_t c = p.c0 + i;
      int32_t o_start = -1, o_len = 0;
      if (live) {
        if (k == 0) {
          // ---- the session's step of call c
          // (its words were loaded a call ahead; the next call's loads go out now)
          const int32_t ll = n_ll, rcv = n_rcv;
          const uint32_t ev_c = n_ev, word_c = n_word;
          load_call(min(i + 1, p.n - 1));
          stopped = ll == kEmitStopped;
          next_old = next;
          pushed = 0;
          int32_t note = 0;
          if (!stopped) {
            // the call's poll: the newest remote frame, then its Event::Disconnected bits (a player's
            // last_frame freezes at its disconnect, p2p_session.rs:618-655)
            recv = p.pkt ? rcv : max(recv, rcv);
            const uint32_t ev = ev_c & rmask & ~disc;
#pragma unroll
            for (int j = 0; j < P; j++)
              if ((ev >> j) & 1u) lf[j] = recv;
            disc |= ev;
            // confirmed_frame (:542-553), before this call's add_local_input
            int32_t confirmed = INT32_MAX;
            if (lbytes) confirmed = ll_prev;
            if (rmask & ~disc) confirmed = min(confirmed, recv);
            if (confirmed == INT32_MAX) confirmed = kNull;  // (no connected player: the session stopped)
            if (lost_call < 0) {
              // the local bytes of the frame this call queued
              if (ll != ll_prev) p.ring[(int64_t)((uint32_t)ll & p.qmask) * S + s] = word_c & lbytes;
              // the remote bytes frame f takes from its input row: the connected players' and those of
              // the players disconnected at or after it (blank_input for the rest)
              uint32_t keep = kAll & ~lbytes;
#pragma unroll
              for (int j = 0; j < P; j++)
                if ((disc >> j) & 1u) keep &= ~(0xffu << (8 * j));
              auto row_bytes = [&](int32_t f) -> uint32_t {
                uint32_t m = keep;
#pragma unroll
                for (int j = 0; j < P; j++)
                  if (((disc >> j) & 1u) && lf[j] >= f) m |= 0xffu << (8 * j);
                return m;
              };
              // 7. every row the burst reads still held?  The oldest frame decides: the rows are lost
              // oldest first, and a later frame reads no byte that an earlier one does not (a frame of
              // blank remote bytes reads none: with every remote player disconnected the confirmed
              // frame runs ahead of the rows)
              if (next <= confirmed && row_bytes(next) && p.row_tag[next % cap] != next) lost_call = c;
              if (lost_call < 0) {
                // 2. confirmed_inputs (sync_layer.rs:296-310)
                int32_t slot = next % cap;  // frame f's row slot, stepped with the frame
                for (int32_t f = next; f <= confirmed; f++) {
                  const uint32_t m = row_bytes(f);
                  uint32_t* cell = p.ring + (int64_t)((uint32_t)f & p.qmask) * S + s;
                  *cell = (*cell & lbytes) | (m ? row_word((int64_t)slot * S + s) & m : 0u);
                  if (++slot == cap) slot = 0;
                }
                if (confirmed >= next) {
                  pushed = confirmed - next + 1;
                  next = confirmed + 1;
                }
              }
            }
            // 5. peer_connect_status: one disconnected player per call, in turn
            if (disc) {
              const int nd = __popc(disc);
              int at = c % nd;
#pragma unroll
              for (int j = 0; j < P; j++)
                if ((disc >> j) & 1u) {
                  if (at == 0) note = 1 | j << 1 | (lf[j] + 1) << 3;
                  --at;
                }
            }
            ll_prev = ll;
          }
          p.o_notes[(int64_t)i * S + s] = note;
        }
        // ---- endpoint k's step of call c (its words selected from the registers: a runtime index
        // would put them in scratch memory)
        int32_t status = 0, la = kNull;
        uint32_t lab = 0;
#pragma unroll
        for (int j = 0; j < kSpecMaxK; j++)
          if (j == k) {
            status = e_status[j];
            la = e_la[j];
            lab = e_lab[j];
          }
        if constexpr (kPoll) {
#pragma unroll
          for (int j = 0; j < kSpecMaxK; j++)
            if (j == k && status == 0 && e_pc[j] >= 0 && e_pc[j] <= c) {
              status = GGRS_EMIT_CLOSED;
              e_status[j] = status;
              e_closed[j] = e_pc[j];
            }
        }
        // (the pair's ack and retry flag were loaded a pair ahead; the next pair's loads go out now)
        const int32_t ack = n_ack;
        const uint32_t rs = n_rs;
        load_pair(min(q + 1, pairs - 1));
        if (!stopped && status == 0) {
          // 1. pop_pending_output (:378-391) over what was pending before the call's pushes
          if (next_old - 1 > la && ack > la) {
            la = min(ack, next_old - 1);
            lab = p.ring[(int64_t)((uint32_t)la & p.qmask) * S + s];
          }
          const int32_t cnt = next - 1 - la;
          int32_t pend = cnt;
          if (lost_call >= 0) {
            status = GGRS_EMIT_ROW_LOST;
          } else if (pushed && cnt > p.maxpend) {
            // 3. send_input's overflow (:443-445): at the first push past max_pending_inputs
            status = GGRS_EMIT_DISCONNECTED;
            pend = p.maxpend + 1;
          } else if (cnt > 0 && (pushed || rs)) {
            // 4. send_pending_output (:450-487)
            uint8_t* row = smem + (size_t)(g * kEmitBlock + t) * pitch;
            // an earlier endpoint of this call with the same last_acked sent the same packet: copy
            // its row if it is still in the group
            int from = -1, from_len = 0;
            if (p.dedup) {
#pragma unroll
              for (int j = 0; j < kSpecMaxK - 1; j++)
                if (j < k && from < 0 && sent_slot[j] >= 0 && e_la[j] == la) {
                  from = sent_slot[j];
                  from_len = sent_len[j];
                }
            }
            if (from >= 0) {
              const uint32_t* src = reinterpret_cast<const uint32_t*>(smem + (size_t)(from * kEmitBlock + t) * pitch);
              uint32_t* dst = reinterpret_cast<uint32_t*>(row);
              for (int w = 0; w < ((from_len + 3) >> 2); w++) dst[w] = src[w];
              o_len = from_len;
            } else {
              RunWriter w{row + kEmitHeader, p.stride - kEmitHeader};
              uint32_t prev = lab;
              for (int32_t f = la + 1; f < next; f++) {
                const uint32_t v = p.ring[(int64_t)((uint32_t)f & p.qmask) * S + s];
                const uint32_t d = v ^ prev;
                prev = v;
#pragma unroll
                for (int b = 0; b < P; b++) w.byte((uint8_t)(d >> (8 * b)));
              }
              w.close();
              o_len = emit_frame_row(row, w.pos, p.stride);
            }
            o_start = la + 1;
          }
#pragma unroll
          for (int j = 0; j < kSpecMaxK; j++)
            if (j == k) {
              e_la[j] = la;
              e_lab[j] = lab;
              e_pend[j] = pend;
              e_status[j] = status;
              if (status) e_closed[j] = c;
              sent_slot[j] = o_len ? g : -1;
              sent_len[j] = o_len;
            }
        } else {
#pragma unroll
          for (int j = 0; j < kSpecMaxK; j++)
            if (j == k) sent_slot[j] = -1;
        }
        const int64_t o = (int64_t)q * S + s;
        p.o_start[o] = o_start;
        p.o_len[o] = o_len;
        need = max(need, (o_len + 3) >> 2);
      }
      l_len[g * kEmitBlock + t] = o_len;
      if (++k == K) {
        k = 0;
        ++i;
      }
    }
    if (need) atomicMax(&s_maxdw, need);
    __syncthreads();
    emit_write_group(smem, l_len, pitch, gn, nb, s_maxdw, p.o_packets, q0, S, s0, p.stride, t);
  }
  if (live) {
    fld(kSpecNext) = next;
    fld(kSpecLlPrev) = ll_prev;
    fld(kSpecRecv) = recv;
    fld(kSpecDisc) = (int32_t)disc;
    fld(kSpecLostCall) = lost_call;
#pragma unroll
    for (int j = 0; j < P; j++) fld(kSpecLf0 + j) = lf[j];
#pragma unroll
    for (int j = 0; j < kSpecMaxK; j++)
      if (j < K) {
        epf(kSpecEpLaFrame, j) = e_la[j];
        epf(kSpecEpLaBytes, j) = (int32_t)e_lab[j];
        epf(kSpecEpPending, j) = e_pend[j];
        epf(kSpecEpStatus, j) = e_status[j];
        epf(kSpecEpClosedCall, j) = e_closed[j];
      }
  }
#undef l_len
}

// GGRS_SPEC_EMIT_DEDUP=0 encodes every endpoint's packet on its own (for the comparison; default 1)
int32_t spec_dedup_from_env() {
  const char* v = std::getenv("GGRS_SPEC_EMIT_DEDUP");
  return !(v && v[0] == '0');
}

}  // namespace

namespace ggrs {

int p2p_spec_emit_free(ggrs_p2p_engine* e) {
  void* bufs[] = {e->spec_ring, e->spec_st, e->spec_ep};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  e->spec_ring = nullptr;
  e->spec_st = nullptr;
  e->spec_ep = nullptr;
  e->spec.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_spectator_emit(ggrs_p2p_engine_t* e, int32_t num_spectators, int32_t max_pending_inputs,
                                int32_t out_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "spectator emit is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "spectator emit needs ggrs_p2p_set_arrival_schedule(e, 1)");
  if (e->peer_reports)
    return set_error(GGRS_E_STATE, "spectator emit with peers' disconnect reports is not supported");
  const int P = e->cfg.num_players;
  if (!(e->cfg.local_mask & ((1 << P) - 1)))
    return set_error(GGRS_E_INVALID, "spectator emit needs a local player (the session that hosts the spectators)");
  if (num_spectators < 1 || num_spectators > 4)
    return set_error(GGRS_E_INVALID, "num_spectators must be in 1..4, got %d", num_spectators);
  if (int rc = PacketEmitState::check(P, max_pending_inputs, out_stride)) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, K = (size_t)num_spectators;
  // the ring holds the slowest open endpoint's pending frames, its last_acked, and the frames queued
  // but not yet confirmed (at most max_prediction + input_delay + 1 ahead of the confirmed one)
  int32_t Q = 1;
  while (Q < max_pending_inputs + e->cfg.max_prediction + e->cfg.input_delay + 2) Q <<= 1;
  if (int rc = p2p_emit_ll_alloc(e)) return rc;
  if (e->spec_ring && (Q != e->spec_q || (int32_t)K != e->spec_k)) {
    HIP_TRY(hipFree(e->spec_ring));
    e->spec_ring = nullptr;
    HIP_TRY(hipFree(e->spec_ep));
    e->spec_ep = nullptr;
  }
  if (!e->spec_st) HIP_TRY(hipMalloc(&e->spec_st, sizeof(int32_t) * (size_t)kSpecFields * S));
  if (!e->spec_ring) {
    HIP_TRY(hipMalloc(&e->spec_ring, sizeof(uint32_t) * (size_t)Q * S));
    HIP_TRY(hipMalloc(&e->spec_ep, sizeof(int32_t) * (size_t)kSpecEpFields * K * S));
  }
  HIP_TRY(hipMemsetAsync(e->spec_ring, 0, sizeof(uint32_t) * (size_t)Q * S, e->stream));
  // every session: nothing confirmed yet, every player connected; every endpoint: nothing
  // acknowledged, nothing pending, the stream open
  if (int rc = emit_fill(e->spec_st, S, kSpecFields, 1u << kSpecNext | 1u << kSpecDisc, e->stream)) return rc;
  constexpr uint32_t kEpZero = 1u << kSpecEpLaBytes | 1u << kSpecEpPending | 1u << kSpecEpStatus;
  if (int rc = emit_fill(e->spec_ep, K * S, kSpecEpFields, kEpZero, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  p2p_spec_poll_free(e);  // (the spectator endpoint poll is configured after this, over these K endpoints)
  e->spec.configure(max_pending_inputs, out_stride);
  e->spec_k = (int32_t)K;
  e->spec_q = Q;
  return GGRS_OK;
}

int ggrs_p2p_emit_spectator_packets(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* ack_in,
                                    const uint8_t* resend, int32_t* start_frame, int32_t* packet_len, int32_t* notes,
                                    uint8_t* packets, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->spec.on) return set_error(GGRS_E_STATE, "emitting spectator packets needs ggrs_p2p_set_spectator_emit");
  if (e->spoll.on && n > 0 && (int64_t)first_call + n > e->spoll.next)
    return set_error(GGRS_E_STATE, "call %d's spectator endpoints were not polled (ggrs_p2p_poll_spectator_endpoints)",
                     std::max(first_call, e->spoll.next));
  const EmitIo io{ack_in, resend, start_frame, packet_len, notes, packets};
  EmitCalls c;
  size_t lds = 0;
  // (a group slot is a (call, endpoint) pair)
  if (int rc = emit_begin(e, e->spec, (size_t)e->spec_k, io, first_call, n, on_device, &c, &lds)) return rc;
  if (n == 0) return GGRS_OK;
  const uint32_t lmask = (uint32_t)e->cfg.local_mask & ((1u << e->cfg.num_players) - 1u);
  const SpecParams p{c.S, c.cap, c.c0, c.n, c.G, e->spec_k, c.maxpend, c.stride, c.Pp, c.pkt, spec_dedup_from_env(),
                     (uint32_t)e->spec_q - 1u, lmask, c.inputs, e->row_tag, c.ll, c.arrive, c.pkt_ack, c.events, c.io.ack_in,
                     c.io.resend, e->spec_ring, e->spec_st, e->spec_ep,
                     e->spoll.on ? e->spoll.st + (size_t)kPollClosedCall * e->spoll.E : nullptr, c.io.start, c.io.len,
                     c.io.word, c.io.packets};
  const int64_t grid = grid_of(c.S, kEmitBlock);
  // (an engine without the spectator endpoint poll launches the kernel it always did)
  auto launch = [&](auto PC) {
    constexpr int PP = decltype(PC)::value;
    if (e->spoll.on) p2p_spec_emit_kernel<PP, true><<<grid, kEmitBlock, lds, e->stream>>>(p);
    else p2p_spec_emit_kernel<PP, false><<<grid, kEmitBlock, lds, e->stream>>>(p);
  };
  switch (e->cfg.num_players) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
  return emit_end(e, e->spec, (size_t)e->spec_k, io, c, on_device);
}

int ggrs_p2p_read_spectator_emit_state(ggrs_p2p_engine_t* e, int32_t* next_spectator_frame, int32_t* last_acked,
                                       int32_t* pending, int32_t* status, int32_t* closed_call) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->spec.on)
    return set_error(GGRS_E_STATE, "the spectator emit state exists with ggrs_p2p_set_spectator_emit only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, KS = (size_t)e->spec_k * S;
  HIP_TRY(read_field(next_spectator_frame, e->spec_st, kSpecNext, S, e->stream));
  auto rd = [&](int32_t* dst, int f) { return read_field(dst, e->spec_ep, f, KS, e->stream); };
  HIP_TRY(rd(last_acked, kSpecEpLaFrame));
  HIP_TRY(rd(pending, kSpecEpPending));
  HIP_TRY(rd(status, kSpecEpStatus));
  HIP_TRY(rd(closed_call, kSpecEpClosedCall));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

}  // extern "C"
