// spectator_ingest.hip -- the packet feed of the spectator engine (spectator.hip): a session's host
// inputs enter as the compressed Input messages its endpoint received, at the call that polled them,
// instead of as dense rows and a recv_upto table known in advance.  This is the receive side of the
// wire protocol, UdpProtocol::on_input (src/network/protocol.rs:564-642), followed by
// SpectatorSession::handle_event's Event::Input (p2p_spectator_session.rs:218-231), for every
// session at once: the packet is checked against last_recv_frame, decoded against the input before
// its first frame (compression::decode, src/network/compression.rs:83-182), its new frames are
// stored into the session's input rows -- the row ring doubles as the endpoint's recv_inputs -- and
// the call's arrival word (recv_upto) and note are written into the grouped tables spectator_kernel
// reads.  The feed is the only writer of a packet-fed engine's rows and tables.
//
// Per session, last_recv starts at NULL_FRAME.  A packet (start, bytes) at call c, in on_input's order:
//   1. gap: last_recv != NULL && last_recv + 1 < start is the reference's assert! (:588-590); a
//      first packet with start != 0 counts as one.  The session stops at call c: the call's arrival
//      word is kSpecFeedStop, which the kFeed form of spectator_kernel turns into GGRS_E_PRECONDITION
//      at that call.  The feed delivers nothing more to a session it stopped.
//   2. reference: the blank input while last_recv == NULL, else all players' bytes of frame start - 1
//      (:594-598), the session's own row.  recv_inputs keeps frames >= last_recv - 2 max_prediction
//      (:636-639): an older start - 1 drops the packet silently (:601-606, GGRS_PACKET_NO_REFERENCE).
//   3. decode (:606): validate_packet's acceptance and codes; all or nothing, no row of a rejected
//      packet is written; more than max_packet_inputs inputs is GGRS_CODEC_E_CAP.
//   4. delivery (:610-631): frames <= last_recv are skipped, every later frame's dword goes into its
//      row, last_recv becomes the packet's last frame.  The host runs on its own clock: no bound by
//      the call.
//   5. recv_upto[c] = ack[c] = last_recv; the call's note goes into the note table whatever became of
//      the packet (:575-585 precedes the decode).
// Why no row tags: a session's delivery is consecutive and gap-free, so slot f % cap holds frame f
// exactly when last_recv - cap < f <= last_recv.  The reference frame start - 1 lies in
// [last_recv - 2 max_prediction, last_recv], inside that window because input_capacity >
// 2 max_prediction + max_packet_inputs (ggrs_spectator_set_packet_feed), and is read before the
// packet's own stores.
//
// Kernel plan (p2p_ingest.hip's where it carries over): one thread per session, one wave per block,
// the block's sessions at the same call -- a session's packets depend on each other through last_recv
// and the reference row.  The block stages its sessions' packets of up to 8 calls at a time into LDS
// with coalesced dword loads, all in flight together (only as many dwords per row as the longest
// packet of the group needs, rows at an odd dword pitch), then per call validates from LDS and expands
// the runs against the previous frame's bytes held in a register.  Every index derived from packet
// bytes is bounded before use (validate_packet).  What differs: every lane is at its own frame and
// ring slot (one modulo per packet, then the slot is stepped); a row is the whole padded dword, so
// delivery is one dword store per frame and the reference one dword load; the kernel writes the
// grouped arrival tables itself.  With hosts on different clocks the 64 row stores of a wave go to up
// to 64 different lines (rows is [cap][S], laid out for spectator_kernel's coalesced reads).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "codec_device.h"
#include "common.h"
#include "spectator_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kIngestBlock = 64;          // sessions (threads) per block: one wave
static_assert(kIngestBlock == 64, "the staging loop splits a group row index by 6 bits");
constexpr int kIngestGroup = 8;           // calls staged at once, at most
constexpr size_t kIngestLds = 64 * 1024;  // a block's packet rows of one call (and their 8 bytes of start, length) must fit
constexpr int32_t kMaxStride = 1012;      // the longest row whose 64 fit, at its odd dword pitch

struct SpecIngestParams {
  int64_t S;
  int32_t cap, acap, maxp, c0, n;
  int32_t G;               // calls staged per group (1 .. kIngestGroup, by the LDS they take)
  int32_t W, stride;       // max_packet_inputs, packet row bytes
  uint32_t* rows;          // [cap][S] one padded dword per (frame, session)
  int32_t* recv;           // [acap / 4][S][4]
  int32_t* notes;          // [acap / 4][S][4]
  const int32_t* start;    // [n][S]
  const int32_t* len;      // [n][S]
  const uint8_t* packets;  // [n][S][stride]
  const int32_t* notes_in; // [n][S] or null
  int32_t* last;           // [S]
  int32_t* stop;           // [S]
  int32_t* status;         // [cap][S]
  int32_t* ack;            // [cap][S]
};

// kP: the players = the bytes of one packet input (compile-time: compression::decode divides the
// stream's 64-bit length by the input size, a few hundred instructions when the divisor is a
// run-time value)
template <int kP>
__global__ __launch_bounds__(kIngestBlock) void spectator_ingest_kernel(SpecIngestParams p) {
  // [G][kIngestBlock][pitch] the packets of a group of calls, then [G][kIngestBlock] their (start, length)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_maxdw;
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int pitch = odd_dword_pitch(p.stride);
  const int64_t s0 = (int64_t)blockIdx.x * kIngestBlock;
  const int nb = (int)min((int64_t)kIngestBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;
  const int32_t cap = p.cap;
  int2* const l_meta = reinterpret_cast<int2*>(smem + (size_t)p.G * kIngestBlock * pitch);
  int32_t last = live ? p.last[s] : kNull;
  int32_t stop = live ? p.stop[s] : 0;  // (a lane without a session: as stopped)

  const int G = p.G;
  int32_t ci = p.c0 % cap;    // the call's slot in the status and ack rings
  int32_t ai = p.c0 % p.acap; // and in the arrival tables
  for (int32_t k0 = 0; k0 < p.n; k0 += G) {
    // ---- a group of calls staged at once: their loads in flight together, one barrier set per group
    const int gn = min(G, p.n - k0);
    __syncthreads();  // (every lane is done with the previous group's rows)
    if (t == 0) s_maxdw = 0;
    int need = 0;
#pragma unroll
    for (int g = 0; g < kIngestGroup; g++) {
      // (unconditional loads, a short group repeating its last call: they issue back to back)
      const int64_t in_i = (int64_t)(k0 + min(g, gn - 1)) * S + s;
      const int32_t st = p.start[in_i], ln = p.len[in_i];
      if (g < gn) {
        l_meta[g * kIngestBlock + t] = make_int2(live ? st : -1, live ? ln : 0);
        if (live && stop == kNull && st >= 0 && ln > 0 && ln <= p.stride) need = max(need, (ln + 3) >> 2);
      }
    }
    __syncthreads();
    if (need) atomicMax(&s_maxdw, need);
    __syncthreads();
    const int maxdw = s_maxdw;  // <= stride / 4
    if (maxdw) {
      // dword q of the group: row (q >> sh) of [gn][kIngestBlock], column q & (2^sh - 1) -- the row
      // length rounded up to a power of two, so that no index needs a division
      const int sh = maxdw > 1 ? 32 - __clz(maxdw - 1) : 0;
      const int sdw = p.stride >> 2, total = (gn * kIngestBlock) << sh;
#pragma unroll 4
      for (int q = t; q < total; q += kIngestBlock) {
        const int row = q >> sh, cc = q & ((1 << sh) - 1);
        const int g = row >> 6, r = row & (kIngestBlock - 1);
        if (cc < maxdw && r < nb) {
          const uint32_t* src = reinterpret_cast<const uint32_t*>(p.packets + ((int64_t)(k0 + g) * S + s0) * p.stride);
          reinterpret_cast<uint32_t*>(smem + row * pitch)[cc] = src[(int64_t)r * sdw + cc];
        }
      }
    }
    __syncthreads();

    for (int g = 0; g < gn; g++) {
      const int32_t k = k0 + g;
      const int32_t c = p.c0 + k;
      const int2 meta = l_meta[g * kIngestBlock + t];
      const int32_t start = meta.x, len = meta.y;
      const bool has = live && stop == kNull && start >= 0;
      // the call's note: a malformed one counts as none (the host path refuses it before the launch)
      int32_t note = (live && p.notes_in) ? p.notes_in[(int64_t)k * S + s] : 0;
      if (!(note & 1) || note < 0 || ((note >> 1) & 3) >= kP) note = 0;

      int32_t status = 0;
      if (has) {
        // 1. the gap (protocol.rs:588-590)
        const bool gap = last == kNull ? start != 0 : last + 1 < start;
        if (gap) {
          status = GGRS_PACKET_STOPPED;
          stop = c;
        } else {
          // 2. the decode reference (:594-606; kept frames :636-639).  start <= last + 1 from here on.
          uint32_t prev = 0;
          bool ok = true;
          const int32_t s_slot = start % cap;  // frame start's row slot (the one modulo of the packet)
          if (last != kNull) {
            const int32_t rf = start - 1;
            if (rf < last - 2 * p.maxp) {
              status = GGRS_PACKET_NO_REFERENCE;
              ok = false;
            } else if (rf >= 0) {
              prev = p.rows[(int64_t)(s_slot == 0 ? cap - 1 : s_slot - 1) * S + s];
            }
          }
          if (ok) {
            // 3. compression::decode's checks (a length outside the row is read nowhere)
            int64_t cnt = 0, rle_at = 0;
            uint64_t m = 0;
            const uint8_t* d = smem + (g * kIngestBlock + t) * pitch;
            status = validate_packet(d, len, p.stride, kP, p.W, &cnt, &m, &rle_at);
            if (status == GGRS_CODEC_OK) {
              // 4. delivery (:610-631): cnt <= W, start <= last + 1, so no overflow
              const int32_t lastf = start + (int32_t)cnt - 1;
              if (cnt > 0 && lastf > last) {
                uint32_t curw = 0;
                int b = 0;
                int32_t f = start, slot = s_slot;
                const int32_t last0 = last;
                expand_runs(d + rle_at, (int64_t)m, [&](uint8_t x) {
                  curw |= (uint32_t)(uint8_t)(x ^ (uint8_t)(prev >> (8 * b))) << (8 * b);
                  if (++b == kP) {
                    if (f > last0 && f <= lastf) p.rows[(int64_t)slot * S + s] = curw;
                    prev = curw;
                    curw = 0;
                    b = 0;
                    ++f;
                    slot = slot + 1 == cap ? 0 : slot + 1;
                  }
                });
                last = lastf;
                status = 1;
              }
            }
          }
        }
      }
      if (live) {
        // 5. the call's results, and its arrival and note words for spectator_kernel
        const int64_t o = (int64_t)ci * S + s;
        p.status[o] = status;
        p.ack[o] = last;
        const int64_t a = (((int64_t)(ai >> 2) * S + s) << 2) + (ai & 3);
        p.recv[a] = stop != kNull ? kSpecFeedStop : last;
        p.notes[a] = note;
      }
      ci = ci + 1 == cap ? 0 : ci + 1;
      ai = ai + 1 == p.acap ? 0 : ai + 1;
    }
  }
  if (live) {
    p.last[s] = last;
    p.stop[s] = stop;
  }
}

int ingest_launch(ggrs_spectator_engine* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                  const int32_t* packet_len, const uint8_t* packets, const int32_t* notes) {
  SpecIngestParams p;
  p.S = e->cfg.num_sessions;
  p.cap = e->cap;
  p.acap = e->acap;
  p.maxp = e->pkt_maxp;
  p.c0 = first_call;
  p.n = n;
  p.W = e->pkt_inputs;
  p.stride = e->pkt_stride;
  p.rows = e->rows;
  p.recv = reinterpret_cast<int32_t*>(e->recv);
  p.notes = reinterpret_cast<int32_t*>(e->notes);
  p.start = start_frame;
  p.len = packet_len;
  p.packets = packets;
  p.notes_in = notes;
  p.last = e->pkt_last;
  p.stop = e->pkt_stop;
  p.status = e->pkt_status;
  p.ack = e->pkt_ack;
  if (int rc = e->timer.before(e->stream)) return rc;
  const size_t per_call = (size_t)kIngestBlock * (odd_dword_pitch(p.stride) + sizeof(int2));
  p.G = (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)kIngestGroup, kIngestLds / per_call, (size_t)n}));
  const size_t lds = p.G * per_call;
  const unsigned grid = (unsigned)grid_of(p.S, kIngestBlock);
  dispatch_players(e->cfg.num_players, [&](auto PC) {
    constexpr int PP = decltype(PC)::value;
    spectator_ingest_kernel<PP><<<grid, kIngestBlock, lds, e->stream>>>(p);
  });
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return GGRS_OK;
}

}  // namespace

namespace ggrs {

int spectator_ingest_free(ggrs_spectator_engine* e) {
  void* bufs[] = {e->pkt_last, e->pkt_stop, e->pkt_status, e->pkt_ack, e->pkt_staging};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  e->pkt_last = e->pkt_stop = e->pkt_status = e->pkt_ack = nullptr;
  e->pkt_staging = nullptr;
  e->pkt_staging_bytes = 0;
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_spectator_set_packet_feed(ggrs_spectator_engine_t* e, int32_t max_prediction, int32_t max_packet_inputs,
                                   int32_t packet_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->calls != 0 || e->next_arrival_call != 0 || e->next_input_frame != 0)
    return set_error(GGRS_E_STATE, "the packet feed is part of the engine's configuration (set before the first input, "
                     "arrival and call)");
  if (max_prediction < 0) return set_error(GGRS_E_INVALID, "max_prediction must be >= 0, got %d", max_prediction);
  if (max_packet_inputs < 1 || max_packet_inputs > 128)
    return set_error(GGRS_E_INVALID, "max_packet_inputs must be in 1..128 (PENDING_OUTPUT_SIZE), got %d", max_packet_inputs);
  const int P = e->cfg.num_players;
  const int32_t need = ggrs_codec_max_packet_bytes(P, max_packet_inputs);
  if (packet_stride < need || packet_stride % 4)
    return set_error(GGRS_E_INVALID, "packet_stride must be a multiple of 4 and >= ggrs_codec_max_packet_bytes(%d, %d) = %d, got %d",
                     P, max_packet_inputs, need, packet_stride);
  if (packet_stride > kMaxStride)
    return set_error(GGRS_E_INVALID, "packet_stride %d is too long (at most %d)", packet_stride, kMaxStride);
  static_assert((size_t)kIngestBlock * (kMaxStride + sizeof(int2)) <= kIngestLds, "one call's rows fit in LDS");
  if ((int64_t)e->cap <= 2 * (int64_t)max_prediction + max_packet_inputs)
    return set_error(GGRS_E_INVALID, "input_capacity %d must exceed 2 * max_prediction + max_packet_inputs = %lld (a packet "
                     "must not reach its own reference's row slot)", e->cap,
                     (long long)(2 * (int64_t)max_prediction + max_packet_inputs));
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)e->cap * S;
  if (!e->pkt_last) {
    HIP_TRY(hipMalloc(&e->pkt_last, sizeof(int32_t) * S));
    HIP_TRY(hipMalloc(&e->pkt_stop, sizeof(int32_t) * S));
    HIP_TRY(hipMalloc(&e->pkt_status, sizeof(int32_t) * rows));
    HIP_TRY(hipMalloc(&e->pkt_ack, sizeof(int32_t) * rows));
  }
  HIP_TRY(hipMemsetAsync(e->pkt_last, 0xff, sizeof(int32_t) * S, e->stream));  // NULL_FRAME
  HIP_TRY(hipMemsetAsync(e->pkt_stop, 0xff, sizeof(int32_t) * S, e->stream));
  HIP_TRY(hipMemsetAsync(e->pkt_status, 0, sizeof(int32_t) * rows, e->stream));
  HIP_TRY(hipMemsetAsync(e->pkt_ack, 0xff, sizeof(int32_t) * rows, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->pkt = 1;
  e->pkt_maxp = max_prediction;
  e->pkt_inputs = max_packet_inputs;
  e->pkt_stride = packet_stride;
  return GGRS_OK;
}

int ggrs_spectator_receive_packets(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                                   const int32_t* packet_len, const uint8_t* packets, const int32_t* notes,
                                   int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->pkt) return set_error(GGRS_E_STATE, "receiving packets needs ggrs_spectator_set_packet_feed");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "packets must be received in call order (expected call %d, got %d)",
                     e->next_arrival_call, first_call);
  if (n == 0) return GGRS_OK;
  if (!start_frame || !packet_len || !packets) return set_error(GGRS_E_INVALID, "null argument");
  if ((int64_t)first_call + n - 1 - e->calls >= e->cap)
    return set_error(GGRS_E_INVALID, "arrival queue full (capacity %d calls)", e->cap);
  if (on_device && ((uintptr_t)packets & 3)) return set_error(GGRS_E_INVALID, "device packets must be dword aligned");
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  if (notes && !on_device) {
    const int P = e->cfg.num_players;
    for (size_t i = 0; i < rows; i++) {
      const int32_t v = notes[i];
      if (v == 0) continue;
      if (!(v & 1) || v < 0 || ((v >> 1) & 3) >= P)
        return set_error(GGRS_E_INVALID, "bad connect-status note %d (call %d, session %lld): GGRS_SPECTATOR_NOTE(player, "
                         "frame) of one of the session's players, frame >= -1", v, first_call + (int32_t)(i / S),
                         (long long)(i % S));
    }
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (!on_device) {  // through the feed's staging buffer: [start][len][notes][packets]
    const size_t bytes = rows * (12 + (size_t)e->pkt_stride);
    if (bytes > e->pkt_staging_bytes) {
      if (e->pkt_staging) HIP_TRY(hipFree(e->pkt_staging));  // (waits for the launches that read it)
      e->pkt_staging = nullptr;
      e->pkt_staging_bytes = 0;
      HIP_TRY(hipMalloc(&e->pkt_staging, bytes));
      e->pkt_staging_bytes = bytes;
    }
    uint8_t* d_start = e->pkt_staging;
    uint8_t* d_len = d_start + 4 * rows;
    uint8_t* d_notes = d_len + 4 * rows;
    uint8_t* d_pk = d_notes + 4 * rows;
    // (stream order keeps an earlier launch's reads of the staging buffer ahead of these copies)
    HIP_TRY(hipMemcpyAsync(d_start, start_frame, 4 * rows, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_len, packet_len, 4 * rows, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_pk, packets, rows * (size_t)e->pkt_stride, hipMemcpyHostToDevice, e->stream));
    if (notes) HIP_TRY(hipMemcpyAsync(d_notes, notes, 4 * rows, hipMemcpyHostToDevice, e->stream));
    start_frame = reinterpret_cast<const int32_t*>(d_start);
    packet_len = reinterpret_cast<const int32_t*>(d_len);
    packets = d_pk;
    if (notes) notes = reinterpret_cast<const int32_t*>(d_notes);
  }
  if (int rc = ingest_launch(e, first_call, n, start_frame, packet_len, packets, notes)) return rc;
  // host sources: the caller may reuse its arrays on return (as ggrs_spectator_add_arrivals); device
  // sources are read in stream order, nothing to wait for
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_arrival_call = first_call + n;
  return GGRS_OK;
}

int ggrs_spectator_read_packet_results(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, int32_t* status,
                                       int32_t* ack_frame) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->pkt) return set_error(GGRS_E_STATE, "packet results exist with ggrs_spectator_set_packet_feed only");
  if (n < 0 || first_call < 0 || (int64_t)first_call + n > e->next_arrival_call ||
      first_call < e->next_arrival_call - e->cap)
    return set_error(GGRS_E_INVALID, "calls %d .. %d are not among the last %d calls received (%d received)",
                     first_call, first_call + n - 1, e->cap, e->next_arrival_call);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int64_t S = e->cfg.num_sessions;
  for (int32_t k = 0; k < n;) {  // rows wrap at cap: at most two pieces
    const int32_t slot = (first_call + k) % e->cap;
    const int32_t m = std::min(n - k, e->cap - slot);
    const size_t off = (size_t)slot * S, dst = (size_t)k * S, cnt = (size_t)m * S;
    if (status) HIP_TRY(hipMemcpyAsync(status + dst, e->pkt_status + off, 4 * cnt, hipMemcpyDeviceToHost, e->stream));
    if (ack_frame) HIP_TRY(hipMemcpyAsync(ack_frame + dst, e->pkt_ack + off, 4 * cnt, hipMemcpyDeviceToHost, e->stream));
    k += m;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

}  // extern "C"
