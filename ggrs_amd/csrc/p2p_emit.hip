// p2p_emit.hip -- the send side of the any-network P2P engine's wire protocol (p2p_sched.hip,
// p2p_ingest.hip): every session's outgoing Input message body is built on the device from the
// engine's own input rows.  This is UdpProtocol::send_input (src/network/protocol.rs:421-448),
// send_pending_output (:450-487), pop_pending_output (:378-391, called from on_input's first line
// :566 and on_input_ack :644-646) and the retry of poll (:333-337), for one endpoint per session
// holding all of its remote players (the packet feed's simplification).
//
// One pending input is B bytes, the local players' bytes of one frame in ascending player order
// (InputBytes::from_inputs, :52-80).  Per session: last_acked = (NULL_FRAME, zeros), pending empty,
// the stream open.  Call c, in the reference's order:
//   1. ack_in[c] pops every pending input with frame <= it; last_acked is the last one popped;
//   2. an Event::Disconnected bit of a remote player closes the stream (GGRS_EMIT_CLOSED);
//   3. if the call's add_local_input was accepted -- the local players' last queued frame, which
//      the scheduled kernels store per call (emit_ll), rose -- that frame is pushed with the local
//      columns of input row c; more than max_pending_inputs pending closes the stream
//      (GGRS_EMIT_DISCONNECTED);
//   4. a packet goes out when a frame was pushed, or resend[c] is set and something is pending:
//      start_frame = the first pending frame, bytes = compression::encode(last_acked, pending...);
//   5. ack_frame[c] = the endpoint's last_recv_frame after the call.
//   6. a stopped session (emit_ll holds kEmitStopped from its stopping call on) takes no step.
// Stated divergences from the reference: the closing call itself emits nothing (there a timer
// resend of the same poll could still go out before the event is handled), and the overflow's
// Event::Disconnected (:443-445) is applied at once, the overflowing call emitting nothing.
//
// One thread per session, one wave per block; the launch's calls are walked in order because
// pending carries from call to call.  pending is a ring in HBM, [128][S], one dword per frame
// (B <= 3: at least one player is remote), slot frame & 127 -- pending frames are consecutive.
// The XOR delta and bitfield-rle's runs (codec.hip's rle_pass: maximal runs of 0x00 / 0xFF
// compressed, maximal stretches of other bytes literal) are produced in one streaming pass from
// registers and the ring into the session's packet row in LDS; a group of calls' rows is then
// written out with coalesced dword stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "codec_device.h"
#include "common.h"
#include "emit_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kRing = kEmitPending;        // PENDING_OUTPUT_SIZE (protocol.rs:22)
static_assert((kRing & (kRing - 1)) == 0, "ring slots are frame & (kRing - 1)");

struct EmitParams {  // (this field order: with the shared EmitCalls block first the kernel measured 1 % slower)
  int64_t S;
  int32_t cap, c0, n, G;
  int32_t maxpend, stride, Pp, pkt;
  uint32_t lpos;               // byte j: the column (player) of local player j in a row word
  uint32_t rmask;              // the remote players' event bits
  const uint8_t* inputs;       // [cap][S] row words
  const int32_t* ll;           // [cap][S] the local players' last queued frame after the call, or kEmitStopped
  const int32_t* arrive;       // [cap][S] (the packet feed off)
  const int32_t* pkt_ack;      // [cap][S] (the packet feed on)
  const uint8_t* events;       // [cap][S]
  const int32_t* ack_in;       // [n][S] or null
  const uint8_t* resend;       // [n][S] or null
  uint32_t* ring;              // [kRing][S]
  int32_t* st;                 // [kEmitFields][S]
  int32_t* o_start;            // [n][S]
  int32_t* o_len;              // [n][S]
  int32_t* o_ack;              // [n][S]
  uint8_t* o_packets;          // [n][S][stride]
};

template <int kB>
__global__ __launch_bounds__(kEmitBlock) void p2p_emit_kernel(EmitParams p) {
  // [G][kEmitBlock][pitch] the packet rows of a group of calls, then [G][kEmitBlock] their lengths
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_maxdw;
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int pitch = odd_dword_pitch(p.stride);
  const int64_t s0 = (int64_t)blockIdx.x * kEmitBlock;
  const int nb = (int)min((int64_t)kEmitBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;  // idle lanes shadow the block's first session, never store
  const int32_t cap = p.cap, Pp = p.Pp;
  constexpr int32_t B = kB;
#define l_len (reinterpret_cast<int32_t*>(smem + (size_t)p.G * kEmitBlock * pitch))
  auto fld = [&](int f) -> int32_t& { return p.st[(int64_t)f * S + s]; };
  int32_t la_frame = fld(kEmitLaFrame), head = fld(kEmitHead), cnt = fld(kEmitCount), status = fld(kEmitStatus);
  int32_t closed = fld(kEmitClosedCall), ll_prev = fld(kEmitLlPrev), recv = fld(kEmitRecv);
  uint32_t la_bytes = (uint32_t)fld(kEmitLaBytes);

  const int G = p.G;
  for (int32_t k0 = 0; k0 < p.n; k0 += G) {
    const int gn = min(G, p.n - k0);
    // the group's per-call words, all loads in flight together (a short group repeats its last call)
    int32_t ll8[kEmitGroup], ack8[kEmitGroup], rcv8[kEmitGroup];
    uint32_t ev8[kEmitGroup], rs8[kEmitGroup], in8[kEmitGroup];
#pragma unroll
    for (int g = 0; g < kEmitGroup; g++) {
      const int32_t k = k0 + min(g, gn - 1);
      const int64_t o = (int64_t)((p.c0 + k) % cap) * S + s, in_i = (int64_t)k * S + s;
      ll8[g] = p.ll[o];
      ev8[g] = p.events[o];
      rcv8[g] = p.pkt ? p.pkt_ack[o] : p.arrive[o];
      ack8[g] = p.ack_in ? p.ack_in[in_i] : kNull;
      rs8[g] = p.resend ? p.resend[in_i] : 0u;
      const uint8_t* w = p.inputs + o * Pp;
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < B; j++) v |= (uint32_t)w[(p.lpos >> (8 * j)) & 0xffu] << (8 * j);
      in8[g] = v;
    }
    __syncthreads();  // (the previous group's rows are written out)
    if (t == 0) s_maxdw = 0;
    __syncthreads();
    int need = 0;
    for (int g = 0; g < gn; g++) {
      const int32_t k = k0 + g;
      const int32_t c = p.c0 + k;
      // this call's words: the front of the batch, which shifts down a call per iteration (indexing
      // it by g would put it in scratch memory)
      const int32_t ll = ll8[0], ack = ack8[0], rcv = rcv8[0];
      const uint32_t ev = ev8[0] & p.rmask, rs = rs8[0], word = in8[0];
#pragma unroll
      for (int j = 0; j < kEmitGroup - 1; j++) {
        ll8[j] = ll8[j + 1];
        ack8[j] = ack8[j + 1];
        rcv8[j] = rcv8[j + 1];
        ev8[j] = ev8[j + 1];
        rs8[j] = rs8[j + 1];
        in8[j] = in8[j + 1];
      }
      int32_t o_start = -1, o_len = 0;
      const bool stopped = ll == kEmitStopped;
      if (!stopped) {
        // 5. last_recv_frame after the call (an arrival row never names a frame after a running call)
        recv = p.pkt ? rcv : max(recv, rcv);
        if (status == 0) {
          // 1. pop_pending_output (:378-391)
          if (cnt > 0 && ack >= head) {
            const int32_t np = min(ack - head + 1, cnt);
            la_frame = head + np - 1;
            la_bytes = p.ring[(int64_t)(la_frame & (kRing - 1)) * S + s];
            head += np;
            cnt -= np;
          }
          const bool pushed = ll != ll_prev;
          if (ev) {
            // 2. disconnect_player_at_frame -> endpoint.disconnect(): send_input returns at :426
            status = GGRS_EMIT_CLOSED;
            closed = c;
          } else {
            // 3. send_input (:421-448)
            if (pushed) {
              if (cnt == 0) head = ll;
              if (live) p.ring[(int64_t)(ll & (kRing - 1)) * S + s] = word;
              ++cnt;
              if (cnt > p.maxpend) {
                status = GGRS_EMIT_DISCONNECTED;
                closed = c;
              }
            }
            // 4. send_pending_output (:450-487)
            if (status == 0 && cnt > 0 && (pushed || rs)) {
              uint8_t* row = smem + (size_t)(g * kEmitBlock + t) * pitch;
              RunWriter w{row + kEmitHeader, p.stride - kEmitHeader};
              uint32_t prev = la_bytes;
              for (int32_t i = 0; i < cnt; i++) {
                const int32_t f = head + i;
                // (the newest frame is this call's word when it was pushed: not yet visible in the ring)
                const uint32_t v = (pushed && i == cnt - 1) ? word : p.ring[(int64_t)(f & (kRing - 1)) * S + s];
                const uint32_t d = v ^ prev;
                prev = v;
#pragma unroll
                for (int b = 0; b < B; b++) w.byte((uint8_t)(d >> (8 * b)));
              }
              w.close();
              o_start = head;
              o_len = emit_frame_row(row, w.pos, p.stride);
            }
          }
        }
        ll_prev = ll;
      }
      l_len[g * kEmitBlock + t] = live ? o_len : 0;
      if (live) need = max(need, (o_len + 3) >> 2);
      if (live) {
        const int64_t o = (int64_t)k * S + s;
        p.o_start[o] = o_start;
        p.o_len[o] = o_len;
        p.o_ack[o] = recv;
      }
    }
    if (need) atomicMax(&s_maxdw, need);
    __syncthreads();
    // ---- the group's rows out, coalesced (emit_device.h)
    emit_write_group(smem, l_len, pitch, gn, nb, s_maxdw, p.o_packets, k0, S, s0, p.stride, t);
  }
  if (live) {
    fld(kEmitLaFrame) = la_frame;
    fld(kEmitLaBytes) = (int32_t)la_bytes;
    fld(kEmitHead) = head;
    fld(kEmitCount) = cnt;
    fld(kEmitStatus) = status;
    fld(kEmitClosedCall) = closed;
    fld(kEmitLlPrev) = ll_prev;
    fld(kEmitRecv) = recv;
  }
#undef l_len
}

int local_players(const ggrs_p2p_engine* e, uint32_t* lpos) {
  int B = 0;
  uint32_t r = 0;
  for (int k = 0; k < e->cfg.num_players; k++)
    if ((e->cfg.local_mask >> k) & 1) {
      if (B < 4) r |= (uint32_t)k << (8 * B);
      B++;
    }
  if (lpos) *lpos = r;
  return B;
}

}  // namespace

namespace ggrs {

int p2p_emit_ll_alloc(ggrs_p2p_engine* e) {
  const size_t rows = (size_t)e->cap * (size_t)e->cfg.num_sessions;
  if (!e->emit_ll) HIP_TRY(hipMalloc(&e->emit_ll, sizeof(int32_t) * rows));
  HIP_TRY(hipMemsetAsync(e->emit_ll, 0xff, sizeof(int32_t) * rows, e->stream));
  return GGRS_OK;
}

int p2p_emit_free(ggrs_p2p_engine* e) {
  void* bufs[] = {e->emit_ll, e->emit_ring, e->emit_st};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  e->emit_ll = nullptr;
  e->emit_ring = nullptr;
  e->emit_st = nullptr;
  e->emit.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_packet_emit(ggrs_p2p_engine_t* e, int32_t max_pending_inputs, int32_t out_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE, "packet emit is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "packet emit needs ggrs_p2p_set_arrival_schedule(e, 1)");
  const int B = local_players(e, nullptr);
  if (B < 1 || B >= e->cfg.num_players)
    return set_error(GGRS_E_INVALID, "packet emit needs a local and a remote player");
  if (int rc = PacketEmitState::check(B, max_pending_inputs, out_stride)) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  if (int rc = p2p_emit_ll_alloc(e)) return rc;
  if (!e->emit_st) {
    HIP_TRY(hipMalloc(&e->emit_ring, sizeof(uint32_t) * (size_t)kEmitPending * S));
    HIP_TRY(hipMalloc(&e->emit_st, sizeof(int32_t) * (size_t)kEmitFields * S));
  }
  HIP_TRY(hipMemsetAsync(e->emit_ring, 0, sizeof(uint32_t) * (size_t)kEmitPending * S, e->stream));
  // every session: nothing acknowledged, nothing pending, the stream open
  constexpr uint32_t kZero = 1u << kEmitLaBytes | 1u << kEmitHead | 1u << kEmitCount | 1u << kEmitStatus;
  if (int rc = emit_fill(e->emit_st, S, kEmitFields, kZero, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->emit.configure(max_pending_inputs, out_stride);
  return GGRS_OK;
}

int ggrs_p2p_emit_packets(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* ack_in,
                          const uint8_t* resend, int32_t* start_frame, int32_t* packet_len, int32_t* ack_frame,
                          uint8_t* packets, int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->emit.on) return set_error(GGRS_E_STATE, "emitting packets needs ggrs_p2p_set_packet_emit");
  const EmitIo io{ack_in, resend, start_frame, packet_len, ack_frame, packets};
  EmitCalls c;
  size_t lds = 0;
  if (int rc = emit_begin(e, e->emit, 1, io, first_call, n, on_device, &c, &lds)) return rc;  // (a group slot is a call)
  if (n == 0) return GGRS_OK;
  uint32_t lpos = 0;
  const int B = local_players(e, &lpos);
  const uint32_t rmask = ~(uint32_t)e->cfg.local_mask & ((1u << e->cfg.num_players) - 1u);
  const EmitParams p{c.S, c.cap, c.c0, c.n, c.G, c.maxpend, c.stride, c.Pp, c.pkt, lpos, rmask, c.inputs, c.ll, c.arrive,
                     c.pkt_ack, c.events, c.io.ack_in, c.io.resend, e->emit_ring, e->emit_st, c.io.start, c.io.len, c.io.word,
                     c.io.packets};
  const int64_t grid = grid_of(c.S, kEmitBlock);
  switch (B) {
    case 1: p2p_emit_kernel<1><<<grid, kEmitBlock, lds, e->stream>>>(p); break;
    case 2: p2p_emit_kernel<2><<<grid, kEmitBlock, lds, e->stream>>>(p); break;
    default: p2p_emit_kernel<3><<<grid, kEmitBlock, lds, e->stream>>>(p); break;
  }
  return emit_end(e, e->emit, 1, io, c, on_device);
}

int ggrs_p2p_read_emit_state(ggrs_p2p_engine_t* e, int32_t* last_acked, int32_t* pending, int32_t* status,
                             int32_t* closed_call) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->emit.on) return set_error(GGRS_E_STATE, "the emit state exists with ggrs_p2p_set_packet_emit only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  auto rd = [&](int32_t* dst, int f) { return read_field(dst, e->emit_st, f, S, e->stream); };
  HIP_TRY(rd(last_acked, kEmitLaFrame));
  HIP_TRY(rd(pending, kEmitCount));
  HIP_TRY(rd(status, kEmitStatus));
  HIP_TRY(rd(closed_call, kEmitClosedCall));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

}  // extern "C"
