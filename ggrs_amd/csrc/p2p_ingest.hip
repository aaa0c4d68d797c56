// p2p_ingest.hip -- the packet feed of the any-network P2P engine (p2p_sched.hip): a session's remote
// inputs enter as the compressed Input messages its endpoint received, at the call that polled
// them, instead of as rows known in advance.  This is the receive side of the wire protocol,
// UdpProtocol::on_input (src/network/protocol.rs:564-642), for every session at once: the packet is
// checked against last_recv_frame, decoded against the input before its first frame
// (compression::decode, src/network/compression.rs:83-182), its new frames are stored into the
// engine's own input rows -- the input ring doubles as the endpoint's recv_inputs -- and the call's
// arrival row (the table ggrs_p2p_add_arrivals takes from the host) is written on the device.  The
// scheduled kernels read the same rows and tables as before.
//
// Per session, last_recv starts at NULL_FRAME.  A packet (start, bytes) at call c, in on_input's order:
//   1. gap: last_recv != NULL && last_recv + 1 < start is the reference's assert! (:588-590); a
//      first packet with start != 0 counts as one (the engine's remote frames start at 0).  The
//      session stops at call c with GGRS_E_PRECONDITION.
//   2. reference: the blank input while last_recv == NULL, else frame start - 1 (:594-598), read
//      from input row start - 1.  recv_inputs keeps frames >= last_recv - 2 max_prediction
//      (:636-639): an older start - 1 drops the packet silently (:601-606, GGRS_PACKET_NO_REFERENCE);
//      a kept one whose row slot holds another frame stops the session (GGRS_E_PRECONDITION, the
//      engine's rule for a remote input no longer in the rows).
//   3. decode (:606): validate_packet's acceptance and codes; all or nothing, no row byte of a
//      rejected packet is written; more than max_packet_inputs inputs is GGRS_CODEC_E_CAP.
//   4. delivery (:610-631): frames <= last_recv are skipped, every later frame's bytes go into the
//      remote columns of its row, last_recv becomes the packet's last frame.  A frame whose row
//      slot holds another frame stops the session (GGRS_E_PRECONDITION); a last frame beyond the
//      call stops it with GGRS_E_INVALID (the arrival table's rule) before anything is stored.
//   5. arrive[c] = last_recv, events[c] = the caller's.
// How a stop reaches the session: the scheduled kernels stop a session at the call whose arrival
// names a frame after it (GGRS_E_INVALID), so a stopping call's arrival row holds such a frame (the
// packet's last frame for 4's case, c + 1 otherwise) and pkt_stop remembers the call; after the
// launch that ran it, ingest_stops_kernel turns that session's error into GGRS_E_PRECONDITION.  The
// feed delivers nothing more to a session it stopped.
//
// One thread per session, one wave per block, the block's sessions at the same call: a session's
// packets depend on each other through last_recv and the reference row.  The block stages its
// sessions' packets of up to 8 calls at a time into LDS with coalesced dword loads, all in flight
// together (only as many dwords per row as the longest packet of the group needs), then per call
// validates from LDS and expands the runs straight into row bytes, XOR-ing against the previous
// frame's bytes held in a register.  Every index derived from packet bytes is bounded before use
// (validate_packet), so hostile bytes never leave the row.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "codec_device.h"
#include "common.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kIngestBlock = 64;               // sessions (threads) per block: one wave
static_assert(kIngestBlock == 64, "the staging loop splits a group row index by 6 bits");
constexpr int kIngestGroup = 8;                // calls staged at once, at most
constexpr int kIngestTags = 2048;              // row tags kept in LDS up to this input_capacity
constexpr size_t kIngestLds = 64 * 1024;       // a block's packet rows of one call (and their 8 bytes of start, length) must fit
constexpr int32_t kStoppedInvalid = -2;        // pkt_stop: <= this, stopped with GGRS_E_INVALID at call -2 - v

struct IngestParams {
  int64_t S;
  int32_t cap, maxp, c0, n;
  int32_t G;                 // calls staged per group (1 .. kIngestGroup, by the LDS they take)
  int32_t tags_lds;          // the row tags are copied to LDS (cap <= kIngestTags and room for them)
  int32_t B, W, stride, Pp;  // remote players (bytes per packet input), max_packet_inputs, packet row bytes, row word bytes
  uint32_t rpos;             // byte j: the column (player) of remote player j in a row word
  uint8_t* inputs;           // [cap][S] row words
  const int32_t* row_tag;    // [cap]
  int32_t* arrive;           // [cap][S]
  uint8_t* events;           // [cap][S]
  const int32_t* start;      // [n][S]
  const int32_t* len;        // [n][S]
  const uint8_t* packets;    // [n][S][stride]
  const uint8_t* ev_in;      // [n][S] or null
  uint32_t ev_mask;          // (1 << num_players) - 1: the bits of ev_in that name a player
  int32_t* last;             // [S]
  int32_t* stop;             // [S]
  int32_t* status;           // [cap][S]
  int32_t* ack;              // [cap][S]
};

// kB: the remote players (compile-time: compression::decode divides the stream's 64-bit length by
// the input size, a few hundred instructions when the divisor is a run-time value)
template <int kB>
__global__ __launch_bounds__(kIngestBlock) void p2p_ingest_kernel(IngestParams p) {
  // [G][kIngestBlock][pitch] the packets of a group of calls, then [G][kIngestBlock] their (start,
  // length), then [cap] the row tags (tags_lds)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_maxdw;
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int pitch = odd_dword_pitch(p.stride);
  const int64_t s0 = (int64_t)blockIdx.x * kIngestBlock;
  const int nb = (int)min((int64_t)kIngestBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;
  const int32_t cap = p.cap, Pp = p.Pp;
  constexpr int32_t B = kB;
#define l_meta (reinterpret_cast<int2*>(smem + (size_t)p.G * kIngestBlock * pitch))
#define l_tags (reinterpret_cast<int32_t*>(smem + (size_t)p.G * kIngestBlock * (pitch + sizeof(int2))))
  // the row tags in LDS when they fit: a session reads several per call, each a memory latency
  // on its chain of calls otherwise
  if (p.tags_lds)
    for (int i = t; i < p.cap; i += kIngestBlock) l_tags[i] = p.row_tag[i];
  // rows are addressed by ring slot, stepped frame by frame: one modulo per packet (an integer
  // modulo by a run-time capacity is some 40 instructions, and a burst would pay it per frame)
  auto tag_at = [&](int32_t slot) -> int32_t { return p.tags_lds ? l_tags[slot] : p.row_tag[slot]; };
  auto next_slot = [&](int32_t slot) -> int32_t { return slot + 1 == cap ? 0 : slot + 1; };
  int32_t last = live ? p.last[s] : kNull;
  int32_t stop = live ? p.stop[s] : kStoppedInvalid;

  // the remote players' bytes of a row word, packed in ascending player order (InputBytes::
  // to_player_inputs over the endpoint's handles, protocol.rs:622), and back
  auto load_remote = [&](int32_t slot) -> uint32_t {
    const uint8_t* w = p.inputs + ((int64_t)slot * S + s) * Pp;
    uint32_t v = 0;
    for (int j = 0; j < B; j++) v |= (uint32_t)w[(p.rpos >> (8 * j)) & 0xffu] << (8 * j);
    return v;
  };
  auto store_remote = [&](int32_t slot, uint32_t v) {
    uint8_t* w = p.inputs + ((int64_t)slot * S + s) * Pp;
    if (B == Pp) {  // every player remote: the whole word
      if (Pp == 1) *w = (uint8_t)v;
      else if (Pp == 2) *reinterpret_cast<uint16_t*>(w) = (uint16_t)v;
      else *reinterpret_cast<uint32_t*>(w) = v;
    } else {
      for (int j = 0; j < B; j++) w[(p.rpos >> (8 * j)) & 0xffu] = (uint8_t)(v >> (8 * j));
    }
  };

  const int G = p.G;
  int32_t ci = p.c0 % cap;  // the call's slot in the arrival rings
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
    const int64_t in_i = (int64_t)k * S + s;
    const int2 meta = l_meta[g * kIngestBlock + t];
    const int32_t start = meta.x, len = meta.y;
    const bool has = live && stop == kNull && start >= 0;

    int32_t status = 0, marker = 0;
    bool stop_now = false;
    if (has) {
      // 1. the gap (protocol.rs:588-590)
      const bool gap = last == kNull ? start != 0 : last + 1 < start;
      if (gap) {
        stop_now = true;
      } else {
        // 2. the decode reference (:594-606; kept frames :636-639)
        uint32_t prev = 0;
        bool ok = true;
        const int32_t s_slot = start % cap;  // frame start's row slot
        if (last != kNull) {
          const int32_t rf = start - 1;
          if (rf < last - 2 * p.maxp) {
            status = GGRS_PACKET_NO_REFERENCE;
            ok = false;
          } else if (rf >= 0) {
            const int32_t rslot = s_slot == 0 ? cap - 1 : s_slot - 1;
            prev = load_remote(rslot);  // (the slot is in the ring whatever it holds)
            if (tag_at(rslot) != rf) {
              stop_now = true;
              ok = false;
            }
          }
        }
        if (ok) {
          // 3. compression::decode's checks (a length outside the row is read nowhere)
          int64_t cnt = 0, rle_at = 0;
          uint64_t m = 0;
          const uint8_t* d = smem + (g * kIngestBlock + t) * pitch;
          status = validate_packet(d, len, p.stride, B, p.W, &cnt, &m, &rle_at);
          if (status == GGRS_CODEC_OK) {
            // 4. delivery (:610-631): cnt <= W, start <= last + 1, so no overflow
            const int32_t lastf = start + (int32_t)cnt - 1;
            if (cnt > 0 && lastf > last) {
              if (lastf > c) {  // a frame the peer cannot have sent yet: the arrival table's rule
                stop_now = true;
                marker = lastf;
              } else {
                bool held = true;
                for (int32_t f = start, slot = s_slot; f <= lastf; ++f, slot = next_slot(slot))
                  if (f > last) held &= tag_at(slot) == f;
                if (!held) {
                  stop_now = true;
                } else {
                  uint32_t curw = 0;
                  int b = 0;
                  int32_t f = start, slot = s_slot;
                  const int32_t last0 = last;
                  expand_runs(d + rle_at, (int64_t)m, [&](uint8_t x) {
                    curw |= (uint32_t)(uint8_t)(x ^ (uint8_t)(prev >> (8 * b))) << (8 * b);
                    if (++b == B) {
                      if (f > last0 && f <= lastf) store_remote(slot, curw);
                      prev = curw;
                      curw = 0;
                      b = 0;
                      ++f;
                      slot = next_slot(slot);
                    }
                  });
                  last = lastf;
                  status = 1;
                }
              }
            }
          }
        }
      }
    }
    if (stop_now) {
      status = GGRS_PACKET_STOPPED;
      stop = marker ? kStoppedInvalid - c : c;
      if (!marker) marker = c + 1;
    }
    if (live) {
      const int64_t o = (int64_t)ci * S + s;
      p.arrive[o] = stop_now ? marker : last;
      // (bits at or above num_players name no player and are dropped here: bit 4 of a stored
      // byte is the scheduled kernels' own peer-report flag)
      p.events[o] = p.ev_in ? (uint8_t)(p.ev_in[in_i] & p.ev_mask) : (uint8_t)0;
      p.status[o] = status;
      p.ack[o] = last;
    }
    ci = next_slot(ci);
   }
  }
  if (live) {
    p.last[s] = last;
    p.stop[s] = stop;
  }
#undef l_meta
#undef l_tags
}

// After a launch of calls: the sessions the feed stopped at a call now run hold the arrival table's
// GGRS_E_INVALID; theirs is the reference's panic.
__global__ void ingest_stops_kernel(int32_t* err, const int32_t* stop, int64_t S, int32_t calls_run) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int32_t st = stop[s];
  if (st >= 0 && st < calls_run && err[s] == GGRS_E_INVALID) err[s] = GGRS_E_PRECONDITION;
}

int remote_players(const ggrs_p2p_engine* e, uint32_t* rpos) {
  int B = 0;
  uint32_t r = 0;
  for (int k = 0; k < e->cfg.num_players; k++)
    if (!((e->cfg.local_mask >> k) & 1)) r |= (uint32_t)k << (8 * B++);
  if (rpos) *rpos = r;
  return B;
}

}  // namespace

namespace ggrs {

int p2p_ingest_free(ggrs_p2p_engine* e) {
  void* bufs[] = {e->pkt_last, e->pkt_stop, e->pkt_status, e->pkt_ack, e->pkt_staging};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  e->pkt_last = e->pkt_stop = e->pkt_status = e->pkt_ack = nullptr;
  e->pkt_staging = nullptr;
  e->pkt_staging_bytes = 0;
  return GGRS_OK;
}

int p2p_ingest_launch(ggrs_p2p_engine* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                      const int32_t* packet_len, const uint8_t* packets, const uint8_t* events) {
  IngestParams p;
  p.S = e->cfg.num_sessions;
  p.cap = e->cap;
  p.maxp = e->cfg.max_prediction;
  p.c0 = first_call;
  p.n = n;
  p.B = remote_players(e, &p.rpos);
  p.W = e->pkt_inputs;
  p.stride = e->pkt_stride;
  p.Pp = e->Pp;
  p.inputs = e->inputs;
  p.row_tag = e->row_tag;
  p.arrive = e->arrive;
  p.events = e->events;
  p.start = start_frame;
  p.len = packet_len;
  p.packets = packets;
  p.ev_in = events;
  p.ev_mask = (1u << e->cfg.num_players) - 1u;
  p.last = e->pkt_last;
  p.stop = e->pkt_stop;
  p.status = e->pkt_status;
  p.ack = e->pkt_ack;
  if (int rc = e->timer.before(e->stream)) return rc;
  const size_t per_call = (size_t)kIngestBlock * (odd_dword_pitch(p.stride) + sizeof(int2));
  size_t tag_bytes = p.cap <= kIngestTags ? sizeof(int32_t) * (size_t)p.cap : 0;
  if (per_call + tag_bytes > kIngestLds) tag_bytes = 0;
  p.tags_lds = tag_bytes != 0;
  p.G = (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)kIngestGroup, (kIngestLds - tag_bytes) / per_call, (size_t)n}));
  const size_t lds = p.G * per_call + tag_bytes;
  const int64_t grid = grid_of(p.S, kIngestBlock);
  switch (p.B) {
    case 1: p2p_ingest_kernel<1><<<grid, kIngestBlock, lds, e->stream>>>(p); break;
    case 2: p2p_ingest_kernel<2><<<grid, kIngestBlock, lds, e->stream>>>(p); break;
    case 3: p2p_ingest_kernel<3><<<grid, kIngestBlock, lds, e->stream>>>(p); break;
    default: p2p_ingest_kernel<4><<<grid, kIngestBlock, lds, e->stream>>>(p); break;
  }
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return GGRS_OK;
}

int p2p_ingest_after_advance(ggrs_p2p_engine* e) {
  const int64_t S = e->cfg.num_sessions;
  ingest_stops_kernel<<<grid_of(S, 256), 256, 0, e->stream>>>(p2p_sched_errors(e), e->pkt_stop, S, e->current_frame);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_packet_feed(ggrs_p2p_engine_t* e, int32_t max_packet_inputs, int32_t packet_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0 || e->next_arrival_call != 0)
    return set_error(GGRS_E_STATE, "the packet feed is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "the packet feed needs ggrs_p2p_set_arrival_schedule(e, 1)");
  const int B = remote_players(e, nullptr);
  if (B < 1) return set_error(GGRS_E_INVALID, "the packet feed needs a remote player");
  if (max_packet_inputs < 1 || max_packet_inputs > 128)
    return set_error(GGRS_E_INVALID, "max_packet_inputs must be in 1..128 (PENDING_OUTPUT_SIZE), got %d", max_packet_inputs);
  const int32_t need = ggrs_codec_max_packet_bytes(B, max_packet_inputs);
  if (packet_stride < need || packet_stride % 4)
    return set_error(GGRS_E_INVALID, "packet_stride must be a multiple of 4 and >= ggrs_codec_max_packet_bytes(%d, %d) = %d, got %d",
                     B, max_packet_inputs, need, packet_stride);
  if ((size_t)kIngestBlock * (odd_dword_pitch(packet_stride) + sizeof(int2)) > kIngestLds)
    return set_error(GGRS_E_INVALID, "packet_stride %d is too long (at most %d)", packet_stride,
                     (int)(kIngestLds / kIngestBlock) - 12);
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
  e->pkt_inputs = max_packet_inputs;
  e->pkt_stride = packet_stride;
  return GGRS_OK;
}

int ggrs_p2p_receive_packets(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                             const int32_t* packet_len, const uint8_t* packets, const uint8_t* events,
                             int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->pkt) return set_error(GGRS_E_STATE, "receiving packets needs ggrs_p2p_set_packet_feed");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "packets must be received in call order (expected call %d, got %d)",
                     e->next_arrival_call, first_call);
  if (n == 0) return GGRS_OK;
  if (!start_frame || !packet_len || !packets) return set_error(GGRS_E_INVALID, "null argument");
  if ((int64_t)first_call + n - 1 - e->current_frame >= e->cap)
    return set_error(GGRS_E_INVALID, "arrival queue full (capacity %d calls)", e->cap);
  if ((int64_t)first_call + n > e->next_input_frame)
    return set_error(GGRS_E_INVALID, "the input rows of calls up to %d must be added first (added up to %d)",
                     first_call + n - 1, e->next_input_frame - 1);
  if (on_device && ((uintptr_t)packets & 3))
    return set_error(GGRS_E_INVALID, "device packets must be dword aligned");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  if (!on_device) {  // through the feed's staging buffer: [start][len][packets][events]
    const size_t bytes = rows * (8 + (size_t)e->pkt_stride + 1);
    if (bytes > e->pkt_staging_bytes) {
      if (e->pkt_staging) HIP_TRY(hipFree(e->pkt_staging));  // (waits for the launches that read it)
      e->pkt_staging = nullptr;
      e->pkt_staging_bytes = 0;
      HIP_TRY(hipMalloc(&e->pkt_staging, bytes));
      e->pkt_staging_bytes = bytes;
    }
    uint8_t* d_start = e->pkt_staging;
    uint8_t* d_len = d_start + 4 * rows;
    uint8_t* d_pk = d_len + 4 * rows;
    uint8_t* d_ev = d_pk + rows * (size_t)e->pkt_stride;
    // (stream order keeps an earlier launch's reads of the staging buffer ahead of these copies)
    HIP_TRY(hipMemcpyAsync(d_start, start_frame, 4 * rows, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_len, packet_len, 4 * rows, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_pk, packets, rows * (size_t)e->pkt_stride, hipMemcpyHostToDevice, e->stream));
    if (events) HIP_TRY(hipMemcpyAsync(d_ev, events, rows, hipMemcpyHostToDevice, e->stream));
    start_frame = reinterpret_cast<const int32_t*>(d_start);
    packet_len = reinterpret_cast<const int32_t*>(d_len);
    packets = d_pk;
    if (events) events = d_ev;
  }
  if (e->peer_reports)  // (a slot's report from cap calls ago is not this call's)
    for (int32_t k = 0; k < n;) {
      const int32_t slot = (first_call + k) % e->cap;
      const int32_t m = std::min(n - k, e->cap - slot);
      HIP_TRY(hipMemsetAsync(e->peer_reports + (int64_t)slot * S, 0, sizeof(int32_t) * m * S, e->stream));
      k += m;
    }
  if (int rc = p2p_ingest_launch(e, first_call, n, start_frame, packet_len, packets, events)) return rc;
  // host sources: the caller may reuse its arrays on return (as ggrs_p2p_add_arrivals); device
  // sources are read in stream order, nothing to wait for
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_arrival_call = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_read_packet_results(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, int32_t* status,
                                 int32_t* ack_frame) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->pkt) return set_error(GGRS_E_STATE, "packet results exist with ggrs_p2p_set_packet_feed only");
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
