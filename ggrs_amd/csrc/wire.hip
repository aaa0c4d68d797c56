// wire.hip -- the GGRS wire envelope, batched and stateless: a poll's raw datagrams become the dense
// arrays the P2P and spectator units take (ggrs_wire_unpack), and the units' output arrays become
// datagrams (ggrs_wire_pack), everything in device memory.
//
// Reference: src/network/messages.rs:5-129 (the message types; MessageBody's variant order is the wire
// tag), UdpProtocol::queue_message / handle_message (src/network/protocol.rs:515-562), on_input's
// envelope part (:564-585), on_input_ack, on_quality_report, on_quality_reply (:644-660) and what the
// send_* functions put into a body (:450-513, :692-698).  A datagram is bincode 1.3's top-level
// serialize of Message (src/network/udp_socket.rs): fixed-width little-endian integers, a u32 enum
// tag, a u64 Vec length, a bool as one byte that must be 0 or 1, a u128 as 16 bytes, fields in
// declaration order, bytes after a complete value accepted:
//   Message            = magic u16 | tag u32 | body
//   Input (0)          = n u64 | n x (disconnected u8, last_frame i32) | disconnect_requested u8
//                        | start_frame i32 | ack_frame i32 | len u64 | bytes[len]
//   InputAck (1)       = ack_frame i32
//   QualityReport (2)  = frame_advantage i16 | ping u128
//   QualityReply (3)   = pong u128
//   ChecksumReport (4) = checksum u128 | frame i32
//   KeepAlive (5)      = nothing
// handle_message never checks the magic (0.10.2 has no sync handshake), so unpack does not either.
//
// Both kernels: one wave per block, one thread per session, the block's sessions at one call.  A
// slot's datagram rows of the block's sessions are contiguous in memory and move between global
// memory and LDS with coalesced dword accesses, only as many dwords per row as the block's longest
// datagram needs (wire_device.h).  Header fields are read from and written to LDS.  An Input's bytes
// sit at offset 31 + 5 n of the datagram, known only once the header is read, and move between that
// unaligned place and the dword-aligned packet row as whole dwords assembled from two neighbours
// (v_alignbyte); the packet rows are staged in LDS as well.  No byte-wise global access, no scratch
// memory.  Every length read from a datagram is compared as u64 and bounded by the datagram's own
// length before it forms an address, so hostile bytes never leave the row.
#include <hip/hip_runtime.h>

#include "common.h"
#include "wire_device.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;

struct UnpackParams {
  int64_t S;
  int32_t n, M, ns, nb, first_call, dstride, pstride;
  uint32_t rmask;
  const uint8_t* dgrams;    // [n][M][S][dstride]
  const int32_t* dlen;      // [n][M][S]
  const uint64_t* now;      // [n]
  int32_t* slot_status;     // [n][M][S]
  int32_t* start;           // [n][S]
  int32_t* plen;            // [n][S]
  uint8_t* packets;         // [n][S][pstride]
  int32_t* ack_in;          // [n][S]
  uint8_t* events;          // [n][S]
  uint8_t* disc;            // [n][S]
  int32_t* last_frame;      // [n][ns][S]
  int32_t* notes;           // [n][S]
  int32_t* radv;            // [n][S]
  uint8_t* ping;            // [n][S][16]
  int32_t* rtt;             // [n][S]
  int32_t* rep_frame;       // [n][S]
  uint16_t* rep_ck;         // [n][S]
  uint8_t* kinds;           // [n][S]
};

// What one (call, session) folds its slots into, in slot order as handle_message would be called
struct Poll {
  int32_t ack_in = kNull, radv = GGRS_TIME_SYNC_KEEP, rtt = -1, rep_frame = kNull;
  int32_t best_start = -1, best_len = 0;
  int32_t lf0 = kNull, lf1 = kNull, lf2 = kNull, lf3 = kNull;
  uint32_t events = 0, disc = 0, kinds = 0, rep_ck = 0;
  uint32_t ping0 = 0, ping1 = 0, ping2 = 0, ping3 = 0;
  bool have_input = false, have_report = false;
};

// One datagram of L bytes (1 <= L <= the row) in the LDS row d: its slot status, and its effect on q.
// prow: the session's packet row in LDS (null: the packets are not wanted).
__device__ inline int32_t unpack_one(const UnpackParams& p, const uint8_t* d, int32_t L, uint64_t now, uint8_t* prow,
                                     Poll& q) {
  if (L < kWireHeader) return GGRS_WIRE_E_BINCODE;
  const uint32_t tag = wire_ld32(d, 2);
  if (tag > (uint32_t)GGRS_WIRE_KEEP_ALIVE) return GGRS_WIRE_E_BINCODE;
  if (tag == GGRS_WIRE_INPUT) {
    if (L < 14) return GGRS_WIRE_E_BINCODE;
    const uint64_t n64 = wire_ld64(d, 6);
    if (n64 > (uint64_t)(L - 14) / 5u) return GGRS_WIRE_E_BINCODE;  // five bytes an element
    const int32_t n = (int32_t)n64;
    uint32_t bad = 0;
    for (int32_t j = 0; j < n; j++) bad |= d[14 + 5 * j];  // every element's bool, the ignored ones too
    const int32_t off = 14 + 5 * n;
    if (L - off < 17) return GGRS_WIRE_E_BINCODE;
    const uint32_t dreq = d[off];
    if ((bad | dreq) > 1u) return GGRS_WIRE_E_BINCODE;
    const int32_t start = (int32_t)wire_ld32(d, off + 1), ack = (int32_t)wire_ld32(d, off + 5);
    const uint64_t m64 = wire_ld64(d, off + 9);
    if (m64 > (uint64_t)(L - off - 17)) return GGRS_WIRE_E_BINCODE;
    if (n < p.ns) return GGRS_WIRE_E_SHAPE;
    if (m64 > (uint64_t)p.pstride) return GGRS_WIRE_E_CAP;
    const int32_t m = (int32_t)m64;
    q.ack_in = max(q.ack_in, ack);
    if (dreq) {
      q.events = p.rmask;
    } else {  // the sticky merge of :577-584 (n >= ns: every element read lies inside the datagram)
      q.disc |= (uint32_t)d[14] & 1u;
      q.lf0 = max(q.lf0, (int32_t)wire_ld32(d, 15));
      if (p.ns > 1) {
        q.disc |= ((uint32_t)d[19] & 1u) << 1;
        q.lf1 = max(q.lf1, (int32_t)wire_ld32(d, 20));
      }
      if (p.ns > 2) {
        q.disc |= ((uint32_t)d[24] & 1u) << 2;
        q.lf2 = max(q.lf2, (int32_t)wire_ld32(d, 25));
      }
      if (p.ns > 3) {
        q.disc |= ((uint32_t)d[29] & 1u) << 3;
        q.lf3 = max(q.lf3, (int32_t)wire_ld32(d, 30));
      }
    }
    if (!q.have_input || start >= q.best_start) {  // the greatest start_frame, ties to the later slot
      q.have_input = true;
      q.best_start = start;
      q.best_len = m;
      if (prow) {
        // bytes [body, body + m) of the datagram -> the packet row's dwords; the last dword's tail is zero
        const int32_t body = off + 17;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(d) + (body >> 2);
        const uint32_t sh = (uint32_t)body & 3u;
        uint32_t* o = reinterpret_cast<uint32_t*>(prow);
        const int32_t nd = (m + 3) >> 2;
        uint32_t lo = w[0];
        for (int32_t k = 0; k < nd; k++) {
          const uint32_t hi = w[k + 1];  // (at most the row's spare dword)
          uint32_t v = wire_align(hi, lo, sh);
          if (k == nd - 1 && (m & 3)) v &= (1u << (8 * (m & 3))) - 1u;
          o[k] = v;
          lo = hi;
        }
      }
    }
  } else if (tag == GGRS_WIRE_INPUT_ACK) {
    if (L < 10) return GGRS_WIRE_E_BINCODE;
    q.ack_in = max(q.ack_in, (int32_t)wire_ld32(d, 6));
  } else if (tag == GGRS_WIRE_QUALITY_REPORT) {
    if (L < 24) return GGRS_WIRE_E_BINCODE;
    q.radv = (int32_t)(int16_t)(uint16_t)(wire_ld32(d, 6) & 0xffffu);
    q.ping0 = wire_ld32(d, 8);
    q.ping1 = wire_ld32(d, 12);
    q.ping2 = wire_ld32(d, 16);
    q.ping3 = wire_ld32(d, 20);
  } else if (tag == GGRS_WIRE_QUALITY_REPLY) {
    if (L < 22) return GGRS_WIRE_E_BINCODE;
    const uint64_t lo = wire_ld64(d, 6), hi = wire_ld64(d, 14);
    if (hi != 0 || lo > now) return GGRS_WIRE_E_CLOCK;  // the assert! of :658
    const uint64_t dt = now - lo;
    q.rtt = dt > (uint64_t)INT32_MAX ? INT32_MAX : (int32_t)dt;
  } else if (tag == GGRS_WIRE_CHECKSUM_REPORT) {
    if (L < 26) return GGRS_WIRE_E_BINCODE;
    const uint64_t lo = wire_ld64(d, 6), hi = wire_ld64(d, 14);
    if (hi != 0 || lo > 0xffffu) return GGRS_WIRE_E_RANGE;
    const int32_t frame = (int32_t)wire_ld32(d, 22);
    if (!q.have_report || frame >= q.rep_frame) {
      q.have_report = true;
      q.rep_frame = frame;
      q.rep_ck = (uint32_t)lo;
    }
  }
  q.kinds |= 1u << tag;
  return (int32_t)tag + 1;
}

__global__ __launch_bounds__(kWireBlock) void wire_unpack_kernel(UnpackParams p) {
  // [nb][dpitch] a slot's datagram rows, [nb][ppitch] the chosen packets' rows, [nb] their lengths
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_max;
  const int t = threadIdx.x, nb = p.nb;
  const int64_t S = p.S, bpc = grid_of(S, nb);
  const int64_t i = (int64_t)blockIdx.x / bpc, s0 = ((int64_t)blockIdx.x % bpc) * nb;
  const int rows = (int)min((int64_t)nb, S - s0);
  const bool live = t < rows;
  const int64_t s = live ? s0 + t : s0;  // idle lanes shadow the block's first session, never store
  const int dpitch = wire_pitch(p.dstride), ppitch = wire_pitch(p.pstride);
  uint8_t* l_d = smem;
  uint8_t* l_p = l_d + (size_t)nb * dpitch;
  int32_t* l_len = reinterpret_cast<int32_t*>(l_p + (size_t)nb * ppitch);
  const uint64_t now = p.now[i];
  Poll q;
  for (int32_t m = 0; m < p.M; m++) {
    const int64_t row0 = (i * p.M + m) * S;
    const int32_t len = live ? p.dlen[row0 + s] : 0;
    const int32_t L = (len > 0 && len <= p.dstride) ? len : 0;  // the bytes read of this row
    const int maxdw = wire_block_max((L + 3) >> 2, &s_max);
    wire_rows_in(l_d, dpitch, p.dgrams + (row0 + s0) * p.dstride, p.dstride, rows, maxdw);
    __syncthreads();
    if (live) {
      int32_t st = 0;
      if (len > p.dstride) st = GGRS_WIRE_E_BINCODE;  // a datagram longer than its buffer
      else if (L) st = unpack_one(p, l_d + (size_t)t * dpitch, L, now, p.packets ? l_p + (size_t)t * ppitch : nullptr, q);
      if (p.slot_status) p.slot_status[row0 + s] = st;
    }
  }
  const int32_t out_len = live && q.have_input ? q.best_len : 0;
  if (t < nb) l_len[t] = out_len;
  const int maxdw = wire_block_max((out_len + 3) >> 2, &s_max);
  if (p.packets) wire_rows_out(p.packets + (i * S + s0) * p.pstride, p.pstride, l_p, ppitch, l_len, rows, maxdw);
  if (!live) return;
  const int64_t o = i * S + s;
  if (p.start) p.start[o] = q.have_input ? q.best_start : -1;
  if (p.plen) p.plen[o] = out_len;
  if (p.ack_in) p.ack_in[o] = q.ack_in;
  if (p.events) p.events[o] = (uint8_t)q.events;
  if (p.disc) p.disc[o] = (uint8_t)q.disc;
  if (p.last_frame) {
    int32_t* lf = p.last_frame + i * p.ns * S + s;
    lf[0] = q.lf0;
    if (p.ns > 1) lf[S] = q.lf1;
    if (p.ns > 2) lf[2 * S] = q.lf2;
    if (p.ns > 3) lf[3 * S] = q.lf3;
  }
  if (p.notes) {
    // the ((first_call + i) mod m)-th disconnected player in ascending order, as
    // ggrs_p2p_emit_spectator_packets rotates its notes
    int32_t note = 0;
    const int cntb = __popc(q.disc);
    if (cntb) {
      int want = (int)(((int64_t)p.first_call + i) % cntb);
      int player = 0;
      int32_t lf = kNull;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool set = (q.disc >> k) & 1u;
        if (set && want == 0) {
          player = k;
          lf = k == 0 ? q.lf0 : (k == 1 ? q.lf1 : (k == 2 ? q.lf2 : q.lf3));
        }
        if (set) --want;
      }
      note = (int32_t)(1u | (uint32_t)player << 1 | ((uint32_t)lf + 1u) << 3);
    }
    p.notes[o] = note;
  }
  if (p.radv) p.radv[o] = q.radv;
  if (p.ping) {
    uint32_t* pg = reinterpret_cast<uint32_t*>(p.ping) + o * 4;
    pg[0] = q.ping0;
    pg[1] = q.ping1;
    pg[2] = q.ping2;
    pg[3] = q.ping3;
  }
  if (p.rtt) p.rtt[o] = q.rtt;
  if (p.rep_frame) p.rep_frame[o] = q.have_report ? q.rep_frame : kNull;
  if (p.rep_ck) p.rep_ck[o] = (uint16_t)(q.have_report ? q.rep_ck : 0u);
  if (p.kinds) p.kinds[o] = (uint8_t)q.kinds;
}

struct PackParams {
  int64_t S;
  int32_t n, ns, nb, dstride, pstride;
  const uint16_t* magic;      // [S]
  const uint64_t* now;        // [n]
  const int32_t* start;       // [n][S]
  const int32_t* plen;        // [n][S]
  const int32_t* ack;         // [n][S]
  const uint8_t* packets;     // [n][S][pstride]
  const uint8_t* disc;        // [n][S]
  const int32_t* last_frame;  // [n][ns][S]
  const uint8_t* dreq;        // [n][S]
  const uint8_t* send_ack;    // [n][S]
  const uint8_t* send_report; // [n][S]
  const int32_t* ladv;        // [n][S]
  const uint8_t* kinds;       // [n][S]
  const uint8_t* ping;        // [n][S][16]
  const int32_t* rep_frame;   // [n][S]
  const uint16_t* rep_ck;     // [n][S]
  const uint8_t* keep;        // [n][S]
  uint8_t* dgrams;            // [n][4][S][dstride]
  int32_t* dlen;              // [n][4][S]
};

__global__ __launch_bounds__(kWireBlock) void wire_pack_kernel(PackParams p) {
  // [nb][dpitch] a slot's datagram rows, [nb][ppitch] the packets' rows, [nb] the datagrams' lengths
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_max;
  const int t = threadIdx.x, nb = p.nb;
  const int64_t S = p.S, bpc = grid_of(S, nb);
  const int64_t i = (int64_t)blockIdx.x / bpc, s0 = ((int64_t)blockIdx.x % bpc) * nb;
  const int rows = (int)min((int64_t)nb, S - s0);
  const bool live = t < rows;
  const int64_t s = live ? s0 + t : s0;
  const int dpitch = wire_pitch(p.dstride), ppitch = wire_pitch(p.pstride);
  uint8_t* l_d = smem;
  uint8_t* l_p = l_d + (size_t)nb * dpitch;
  int32_t* l_len = reinterpret_cast<int32_t*>(l_p + (size_t)nb * ppitch);
  uint8_t* row = l_d + (size_t)t * dpitch;
  uint32_t* w = reinterpret_cast<uint32_t*>(row);
  const int64_t o = i * S + s;
  // the call's words, all loads in flight together
  const uint32_t magic = p.magic[s];
  const uint64_t now = p.now[i];
  const bool has_in = p.start && p.plen && p.packets;
  const int32_t start = has_in ? p.start[o] : -1, plen = has_in ? p.plen[o] : 0;
  const int32_t ack = p.ack ? p.ack[o] : kNull;
  const uint32_t disc = p.disc ? p.disc[o] : 0u, dreq = p.dreq ? p.dreq[o] : 0u;
  const bool send_ack = p.send_ack && p.send_ack[o], send_report = p.send_report && p.send_report[o];
  const int32_t ladv = p.ladv ? p.ladv[o] : 0;
  const bool reply = p.kinds && ((p.kinds[o] >> GGRS_WIRE_QUALITY_REPORT) & 1u);
  const int32_t rep_frame = p.rep_frame ? p.rep_frame[o] : kNull;
  const uint32_t rep_ck = p.rep_ck ? p.rep_ck[o] : 0u;
  const bool keep = p.keep && p.keep[o];
  const bool input = live && start >= 0 && plen > 0 && plen <= p.pstride;
  auto header = [&](uint32_t tag) { w[0] = magic | tag << 16; };  // (the tag's upper half is zero: dword 1)
  auto emit = [&](int m, int32_t len) {  // the slot's rows out, then the rows are free again
    if (t < nb) l_len[t] = live ? len : 0;
    const int maxdw = wire_block_max(live ? (len + 3) >> 2 : 0, &s_max);
    wire_rows_out(p.dgrams + ((i * 4 + m) * S + s0) * p.dstride, p.dstride, l_d, dpitch, l_len, rows, maxdw);
    if (live) p.dlen[(i * 4 + m) * S + s] = len;
    __syncthreads();
  };

  // ---- slot 0: Input, else InputAck, else KeepAlive when nothing else goes out
  {
    const int maxdw = wire_block_max(input ? (plen + 3) >> 2 : 0, &s_max);
    if (has_in) wire_rows_in(l_p, ppitch, p.packets + (i * S + s0) * p.pstride, p.pstride, rows, maxdw);
    __syncthreads();
    int32_t len = 0;
    if (input) {
      header(GGRS_WIRE_INPUT);
      w[1] = (uint32_t)p.ns << 16;  // peer_connect_status' length, a u64 from byte 6
      w[2] = 0;
      w[3] = 0;
      int32_t off = 14;
      for (int k = 0; k < p.ns; k++) {
        row[off] = (uint8_t)((disc >> k) & 1u);
        wire_st32(row, off + 1, (uint32_t)(p.last_frame ? p.last_frame[(i * p.ns + k) * S + s] : kNull));
        off += 5;
      }
      row[off] = dreq ? 1 : 0;
      wire_st32(row, off + 1, (uint32_t)start);
      wire_st32(row, off + 5, (uint32_t)ack);
      wire_st32(row, off + 9, (uint32_t)plen);
      wire_st32(row, off + 13, 0u);
      off += 17;  // 31 + 5 ns: where the bytes start
      // the packet row's dwords -> bytes [off, off + plen): each datagram dword from two neighbours
      const uint32_t* src = reinterpret_cast<const uint32_t*>(l_p + (size_t)t * ppitch);
      const int32_t base = off >> 2;
      const uint32_t sh = (uint32_t)off & 3u;
      const int32_t nd = ((int32_t)sh + plen + 3) >> 2;
      uint32_t carry = sh ? w[base] << (8 * (4 - sh)) : 0u;  // the header's last bytes, on top
      for (int32_t k = 0; k < nd; k++) {
        const uint32_t v = src[k];  // (at most the packet row's spare dword)
        w[base + k] = sh ? wire_align(v, carry, 4 - sh) : v;
        carry = v;
      }
      len = off + plen;
    } else if (live && send_ack) {
      header(GGRS_WIRE_INPUT_ACK);
      w[1] = (uint32_t)ack << 16;
      w[2] = (uint32_t)ack >> 16;
      len = 10;
    } else if (live && keep && !send_report && !reply && rep_frame < 0) {
      header(GGRS_WIRE_KEEP_ALIVE);
      w[1] = 0;
      len = 6;
    }
    emit(0, len);
  }
  // ---- slot 1: QualityReport{clamp_i16(local_advantage), ping = now_ms}
  {
    int32_t len = 0;
    if (live && send_report) {
      const int32_t adv = min(max(ladv, -32768), 32767);
      header(GGRS_WIRE_QUALITY_REPORT);
      w[1] = ((uint32_t)adv & 0xffffu) << 16;
      w[2] = (uint32_t)now;
      w[3] = (uint32_t)(now >> 32);
      w[4] = 0;
      w[5] = 0;
      len = 24;
    }
    emit(1, len);
  }
  // ---- slot 2: QualityReply{pong = the ping unpack kept}
  {
    int32_t len = 0;
    if (live && reply) {
      uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0;
      if (p.ping) {
        const uint32_t* pg = reinterpret_cast<const uint32_t*>(p.ping) + o * 4;
        g0 = pg[0];
        g1 = pg[1];
        g2 = pg[2];
        g3 = pg[3];
      }
      header(GGRS_WIRE_QUALITY_REPLY);
      w[1] = g0 << 16;
      w[2] = wire_align(g1, g0, 2);
      w[3] = wire_align(g2, g1, 2);
      w[4] = wire_align(g3, g2, 2);
      w[5] = g3 >> 16;
      len = 22;
    }
    emit(2, len);
  }
  // ---- slot 3: ChecksumReport{checksum as u128, frame}
  {
    int32_t len = 0;
    if (live && rep_frame >= 0) {
      header(GGRS_WIRE_CHECKSUM_REPORT);
      w[1] = rep_ck << 16;
      w[2] = 0;
      w[3] = 0;
      w[4] = 0;
      w[5] = (uint32_t)rep_frame << 16;
      w[6] = (uint32_t)rep_frame >> 16;
      len = 26;
    }
    emit(3, len);
  }
}

bool aligned4(const void* a) { return ((uintptr_t)a & 3) == 0; }

int check_strides(int32_t num_statuses, int32_t dgram_stride, int32_t packet_stride) {
  if (num_statuses < 1 || num_statuses > 4)
    return set_error(GGRS_E_INVALID, "wire: num_statuses must be in 1..4, got %d", num_statuses);
  if (packet_stride < 4 || packet_stride > kWireMaxPacket || packet_stride % 4)
    return set_error(GGRS_E_INVALID, "wire: packet_stride must be a multiple of 4 in 4..%d, got %d", kWireMaxPacket,
                     packet_stride);
  if (dgram_stride < 8 || dgram_stride > kWireMaxDgram || dgram_stride % 4)
    return set_error(GGRS_E_INVALID, "wire: dgram_stride must be a multiple of 4 in 8..%d, got %d", kWireMaxDgram,
                     dgram_stride);
  return GGRS_OK;
}

}  // namespace

extern "C" {

int32_t ggrs_wire_max_datagram_bytes(int32_t num_statuses, int32_t body_bytes) {
  const int64_t v = ((int64_t)kWireInputFixed + 5 * (int64_t)num_statuses + body_bytes + 15) / 16 * 16;
  return num_statuses < 0 || body_bytes < 0 || v > 0x7fffffff ? -1 : (int32_t)v;
}

int ggrs_wire_unpack(int32_t n_calls, int32_t num_sessions, int32_t slots, int32_t num_statuses, uint32_t remote_mask,
                     int32_t first_call, const uint8_t* dgrams, int32_t dgram_stride, const int32_t* dgram_len,
                     const uint64_t* now_ms, int32_t packet_stride, int32_t* slot_status, int32_t* start_frame,
                     int32_t* packet_len, uint8_t* packets, int32_t* ack_in, uint8_t* events, uint8_t* disc_mask,
                     int32_t* last_frame, int32_t* notes, int32_t* remote_advantage, uint8_t* ping, int32_t* rtt_ms,
                     int32_t* report_frame, uint16_t* report_checksum, uint8_t* kinds, void* stream) {
  if (n_calls < 0 || num_sessions < 1 || first_call < 0)
    return set_error(GGRS_E_INVALID, "wire: need n_calls >= 0, num_sessions >= 1, first_call >= 0");
  if (slots < 1 || slots > 8) return set_error(GGRS_E_INVALID, "wire: slots per poll must be in 1..8, got %d", slots);
  if (int rc = check_strides(num_statuses, dgram_stride, packet_stride)) return rc;
  if (n_calls == 0) return GGRS_OK;
  if (!dgrams || !dgram_len || !now_ms) return set_error(GGRS_E_INVALID, "wire: null dgrams, dgram_len or now_ms");
  if (!aligned4(dgrams) || !aligned4(packets) || !aligned4(ping))
    return set_error(GGRS_E_INVALID, "wire: dgrams, packets and ping must be dword aligned");
  const int nb = wire_sessions_per_block(dgram_stride, packet_stride);
  const int64_t grid = grid_of(num_sessions, nb) * n_calls;
  if (grid > 0x7fffffff) return set_error(GGRS_E_INVALID, "wire: too many (call, session) blocks for one launch");
  const UnpackParams p{num_sessions, n_calls, slots, num_statuses, nb, first_call, dgram_stride, packet_stride,
                       remote_mask, dgrams, dgram_len, now_ms, slot_status, start_frame, packet_len, packets, ack_in,
                       events, disc_mask, last_frame, notes, remote_advantage, ping, rtt_ms, report_frame,
                       report_checksum, kinds};
  wire_unpack_kernel<<<(unsigned)grid, kWireBlock, wire_lds_bytes(nb, dgram_stride, packet_stride), (hipStream_t)stream>>>(p);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

int ggrs_wire_pack(int32_t n_calls, int32_t num_sessions, int32_t num_statuses, const uint16_t* magic,
                   const uint64_t* now_ms, const int32_t* start_frame, const int32_t* packet_len,
                   const int32_t* ack_frame, const uint8_t* packets, int32_t packet_stride, const uint8_t* disc_mask,
                   const int32_t* last_frame, const uint8_t* disconnect_requested, const uint8_t* send_ack,
                   const uint8_t* send_report, const int32_t* local_advantage, const uint8_t* kinds, const uint8_t* ping,
                   const int32_t* report_frame, const uint16_t* report_checksum, const uint8_t* keep_alive,
                   uint8_t* dgrams, int32_t dgram_stride, int32_t* dgram_len, void* stream) {
  if (n_calls < 0 || num_sessions < 1) return set_error(GGRS_E_INVALID, "wire: need n_calls >= 0, num_sessions >= 1");
  if (int rc = check_strides(num_statuses, dgram_stride, packet_stride)) return rc;
  if (dgram_stride < ggrs_wire_max_datagram_bytes(num_statuses, packet_stride))
    return set_error(GGRS_E_INVALID, "wire: dgram_stride %d < ggrs_wire_max_datagram_bytes(%d, %d) = %d", dgram_stride,
                     num_statuses, packet_stride, ggrs_wire_max_datagram_bytes(num_statuses, packet_stride));
  if (n_calls == 0) return GGRS_OK;
  if (!magic || !now_ms || !dgrams || !dgram_len) return set_error(GGRS_E_INVALID, "wire: null magic, now_ms, dgrams or dgram_len");
  if (!aligned4(dgrams) || !aligned4(packets) || !aligned4(ping))
    return set_error(GGRS_E_INVALID, "wire: dgrams, packets and ping must be dword aligned");
  const int nb = wire_sessions_per_block(dgram_stride, packet_stride);
  const int64_t grid = grid_of(num_sessions, nb) * n_calls;
  if (grid > 0x7fffffff) return set_error(GGRS_E_INVALID, "wire: too many (call, session) blocks for one launch");
  const PackParams p{num_sessions, n_calls, num_statuses, nb, dgram_stride, packet_stride, magic, now_ms, start_frame,
                     packet_len, ack_frame, packets, disc_mask, last_frame, disconnect_requested, send_ack, send_report,
                     local_advantage, kinds, ping, report_frame, report_checksum, keep_alive, dgrams, dgram_len};
  wire_pack_kernel<<<(unsigned)grid, kWireBlock, wire_lds_bytes(nb, dgram_stride, packet_stride), (hipStream_t)stream>>>(p);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

}  // extern "C"
