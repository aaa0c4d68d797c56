// ingest_device.h -- the receive side of the wire protocol shared by the two packet feeds,
// p2p_ingest.hip (a P2P session's remote inputs) and spectator_ingest.hip (a spectator's host inputs):
// UdpProtocol::on_input (src/network/protocol.rs:564-642) up to the delivery of a packet's new frames,
// for every session at once, and the kernel plan around it.  Wire format: see codec.hip.
//
// Per session, last_recv starts at NULL_FRAME.  A packet (start, bytes) at call c, in on_input's order:
//   1. gap: last_recv != NULL && last_recv + 1 < start is the reference's assert! (:588-590); a first
//      packet with start != 0 counts as one (frames start at 0).  The session stops at call c.
//   2. reference: the blank input while last_recv == NULL, else frame start - 1 (:594-598), read from
//      the feed's own rows.  recv_inputs keeps frames >= last_recv - 2 max_prediction (:636-639): an
//      older start - 1 drops the packet silently (:601-606, GGRS_PACKET_NO_REFERENCE); a kept one
//      the rows no longer hold stops the session.
//   3. decode (:606): validate_packet's acceptance and codes; all or nothing, no row of a rejected
//      packet is written; more than max_packet_inputs inputs is GGRS_CODEC_E_CAP.
//   4. delivery (:610-631): frames <= last_recv are skipped, every later frame is stored into its row,
//      last_recv becomes the packet's last frame -- unless the feed refuses the delivery, which stops
//      the session before anything is stored.
// The call's status and ack (last_recv after it) go into their [cap][S] rings; a stopping call's
// status is GGRS_PACKET_STOPPED, and the feed delivers nothing more to a session it stopped.
//
// What a feed supplies is its row policy (`Rows` below): where an input's bytes live, whether a row
// slot still holds its frame, what else bounds a delivery, and the call's other outputs.
//
// Kernel plan: one thread per session, one wave per block, the block's sessions at the same call -- a
// session's packets depend on each other through last_recv and the reference row.  The block stages
// its sessions' packets of up to 8 calls at a time into LDS with coalesced dword loads, all in flight
// together (only as many dwords per row as the longest packet of the group needs, rows at an odd
// dword pitch), then per call validates from LDS and expands the runs straight into row words,
// XOR-ing against the previous frame's bytes held in a register.  Rows are addressed by ring slot,
// stepped frame by frame: one modulo per packet (an integer modulo by a run-time capacity is some 40
// instructions, and a burst would pay it per frame).  Every index derived from packet bytes is
// bounded before use (validate_packet), so hostile bytes never leave the row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "codec_device.h"
#include "common.h"

namespace ggrs {
namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kIngestBlock = 64;  // sessions (threads) per block: one wave
static_assert(kIngestBlock == 64, "the staging loop splits a group row index by 6 bits");
constexpr int kIngestGroup = 8;           // calls staged at once, at most
constexpr size_t kIngestLds = 64 * 1024;  // a block's packet rows of one call (and their 8 bytes of start, length) must fit
constexpr int32_t kIngestMaxStride = 1012;  // the longest row whose 64 fit, at its odd dword pitch

// LDS of one staged call: the block's packet rows and their (start, length)
constexpr size_t ingest_call_bytes(int32_t stride) { return (size_t)kIngestBlock * (odd_dword_pitch(stride) + sizeof(int2)); }
static_assert(ingest_call_bytes(kIngestMaxStride) <= kIngestLds && ingest_call_bytes(kIngestMaxStride + 4) > kIngestLds,
              "one call's rows fit in LDS");

// The calls staged per group and the launch's dynamic LDS for rows of `stride` bytes and n calls;
// `extra` bytes of the feed's own follow the group (their room is the caller's to check)
struct IngestPlan {
  int32_t G;
  size_t lds;
};
inline IngestPlan ingest_plan(int32_t stride, int32_t n, size_t extra) {
  const size_t per_call = ingest_call_bytes(stride);
  const size_t G = std::max<size_t>(1, std::min<size_t>({(size_t)kIngestGroup, (kIngestLds - extra) / per_call, (size_t)n}));
  return {(int32_t)G, G * per_call + extra};
}

// What both kernels take
struct IngestFeed {
  int64_t S;
  int32_t cap, maxp, c0, n;
  int32_t G;               // calls staged per group (1 .. kIngestGroup, by the LDS they take)
  int32_t W, stride;       // max_packet_inputs, packet row bytes
  const int32_t* start;    // [n][S]
  const int32_t* len;      // [n][S]
  const uint8_t* packets;  // [n][S][stride]
  int32_t* last;           // [S]
  int32_t* stop;           // [S] NULL_FRAME while the feed runs, else the feed's own word
  int32_t* status;         // [cap][S]
  int32_t* ack;            // [cap][S]
};

// ... filled from the engine's feed state for a launch of calls c0 .. c0 + n - 1 (device pointers)
inline IngestFeed ingest_feed(const PacketFeedState& f, int64_t S, int32_t cap, int32_t maxp, int32_t c0, int32_t n,
                              int32_t G, const int32_t* start, const int32_t* len, const uint8_t* packets) {
  return {S, cap, maxp, c0, n, G, f.inputs, f.stride, start, len, packets, f.last, f.stop, f.status, f.ack};
}

// A thread's place in its block, and the block's LDS: [G][kIngestBlock][pitch] the packets of a group
// of calls, then [G][kIngestBlock] their (start, length), then what the feed keeps there itself
struct IngestLane {
  int t, nb;      // the thread; the block's sessions (fewer than kIngestBlock in the last block)
  bool live;      // the thread has a session
  int64_t s0, s;  // the block's first session; the thread's (s0 without one: its loads stay in bounds)
  int pitch;
  uint8_t* l_rows;
  int2* l_meta;
  uint8_t* l_own;
  __device__ inline IngestLane(const IngestFeed& p, uint8_t* smem) {
    t = threadIdx.x;
    pitch = odd_dword_pitch(p.stride);
    s0 = (int64_t)blockIdx.x * kIngestBlock;
    nb = (int)min((int64_t)kIngestBlock, p.S - s0);
    live = t < nb;
    s = live ? s0 + t : s0;
    l_rows = smem;
    l_meta = reinterpret_cast<int2*>(smem + (size_t)p.G * kIngestBlock * pitch);
    l_own = smem + (size_t)p.G * kIngestBlock * (pitch + sizeof(int2));
  }
};

// Calls k0 .. k0 + gn - 1 staged at once: their loads in flight together, one barrier set per group.
// `running`: the thread's session takes packets (it has one, and the feed has not stopped it).
__device__ inline void ingest_stage_group(const IngestFeed& p, const IngestLane& b, int32_t k0, int gn, bool running) {
  __shared__ int s_maxdw;
  __syncthreads();  // (every lane is done with the previous group's rows)
  if (b.t == 0) s_maxdw = 0;
  int need = 0;
#pragma unroll
  for (int g = 0; g < kIngestGroup; g++) {
    // (unconditional loads, a short group repeating its last call: they issue back to back)
    const int64_t in_i = (int64_t)(k0 + min(g, gn - 1)) * p.S + b.s;
    const int32_t st = p.start[in_i], ln = p.len[in_i];
    if (g < gn) {
      b.l_meta[g * kIngestBlock + b.t] = make_int2(b.live ? st : -1, b.live ? ln : 0);
      if (running && st >= 0 && ln > 0 && ln <= p.stride) need = max(need, (ln + 3) >> 2);
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
    for (int q = b.t; q < total; q += kIngestBlock) {
      const int row = q >> sh, cc = q & ((1 << sh) - 1);
      const int g = row >> 6, r = row & (kIngestBlock - 1);
      if (cc < maxdw && r < b.nb) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.packets + ((int64_t)(k0 + g) * p.S + b.s0) * p.stride);
        reinterpret_cast<uint32_t*>(b.l_rows + row * b.pitch)[cc] = src[(int64_t)r * sdw + cc];
      }
    }
  }
  __syncthreads();
}

// A feed's answer to "may frames (last .. lastf] be delivered at call c?"
enum class IngestDelivery { kDeliver, kStop, kStopBeyondCall };

// What became of a call's packet: its status; whether it stops the session, and then the packet's
// last frame where that frame, beyond the call, is the reason (0 otherwise)
struct IngestOutcome {
  int32_t status = 0;
  bool stopped = false;
  int32_t marker = 0;
};

// on_input steps 1-4 for one session's packet of call c: `d` its bytes in LDS, `last` the session's
// last_recv.  kB: the bytes of one packet input (compile-time: compression::decode divides the
// stream's 64-bit length by the input size, a few hundred instructions when the divisor is a
// run-time value).  Rows, the feed's row policy, answers for this thread's session:
//   uint32_t load_reference(rslot, rf, held)   the input word in row slot rslot, and whether the slot
//                                              holds frame rf (the slot is in the ring whatever it holds)
//   IngestDelivery check_delivery(start, s_slot, last, lastf, c)
//                                              s_slot: frame start's row slot
//   void store(slot, word)                     a delivered frame's input word
// (and the per-call hooks of ingest_walk).
template <int kB, typename Rows>
__device__ inline IngestOutcome ingest_on_input(const IngestFeed& p, Rows& rows, const uint8_t* d, int32_t start,
                                                int32_t len, int32_t c, int32_t& last) {
  IngestOutcome r;
  const int32_t cap = p.cap;
  // 1. the gap (protocol.rs:588-590)
  if (last == kNull ? start != 0 : last + 1 < start) {
    r.stopped = true;
    return r;
  }
  // 2. the decode reference (:594-606; kept frames :636-639).  start <= last + 1 from here on.
  uint32_t prev = 0;
  const int32_t s_slot = start % cap;  // frame start's row slot (the one modulo of the packet)
  if (last != kNull) {
    const int32_t rf = start - 1;
    if (rf < last - 2 * p.maxp) {
      r.status = GGRS_PACKET_NO_REFERENCE;
      return r;
    }
    if (rf >= 0) {
      bool held = true;
      prev = rows.load_reference(s_slot == 0 ? cap - 1 : s_slot - 1, rf, held);
      if (!held) {
        r.stopped = true;
        return r;
      }
    }
  }
  // 3. compression::decode's checks (a length outside the row is read nowhere)
  int64_t cnt = 0, rle_at = 0;
  uint64_t m = 0;
  r.status = validate_packet(d, len, p.stride, kB, p.W, &cnt, &m, &rle_at);
  if (r.status != GGRS_CODEC_OK) return r;
  // 4. delivery (:610-631): cnt <= W, start <= last + 1, so no overflow
  const int32_t lastf = start + (int32_t)cnt - 1;
  if (cnt <= 0 || lastf <= last) return r;
  const IngestDelivery how = rows.check_delivery(start, s_slot, last, lastf, c);
  if (how != IngestDelivery::kDeliver) {
    r.stopped = true;
    if (how == IngestDelivery::kStopBeyondCall) r.marker = lastf;
    return r;
  }
  uint32_t curw = 0;
  int b = 0;
  int32_t f = start, slot = s_slot;
  const int32_t last0 = last;
  expand_runs(d + rle_at, (int64_t)m, [&](uint8_t x) {
    curw |= (uint32_t)(uint8_t)(x ^ (uint8_t)(prev >> (8 * b))) << (8 * b);
    if (++b == kB) {
      if (f > last0 && f <= lastf) rows.store(slot, curw);
      prev = curw;
      curw = 0;
      b = 0;
      ++f;
      slot = slot + 1 == cap ? 0 : slot + 1;
    }
  });
  last = lastf;
  r.status = 1;
  return r;
}

// A launch's n calls for the block's sessions: every group staged, every call's packet through
// on_input, the call's status and ack written, last_recv and the stop word kept across launches.
// Rows' per-call hooks:
//   void begin_call(k)                          before call k's packet (what the feed loads early)
//   void write_outputs(k, c, o, r, last, stop)  a thread with a session: the feed's own outputs of call
//                                               c = c0 + k (o: its index in the [cap][S] rings), and
//                                               `stop` set in the feed's encoding where r.stopped
template <int kB, typename Rows>
__device__ inline void ingest_walk(const IngestFeed& p, const IngestLane& b, Rows& rows) {
  const int32_t cap = p.cap;
  int32_t last = b.live ? p.last[b.s] : kNull;
  int32_t stop = b.live ? p.stop[b.s] : 0;  // (a lane without a session: as stopped)
  const int G = p.G;
  int32_t ci = p.c0 % cap;  // the call's slot in the status and ack rings
  for (int32_t k0 = 0; k0 < p.n; k0 += G) {
    const int gn = min(G, p.n - k0);
    ingest_stage_group(p, b, k0, gn, b.live && stop == kNull);
    for (int g = 0; g < gn; g++) {
      const int32_t k = k0 + g;
      const int32_t c = p.c0 + k;
      const int2 meta = b.l_meta[g * kIngestBlock + b.t];
      const int32_t start = meta.x, len = meta.y;
      rows.begin_call(k);
      IngestOutcome r;
      if (b.live && stop == kNull && start >= 0)
        r = ingest_on_input<kB>(p, rows, b.l_rows + (g * kIngestBlock + b.t) * b.pitch, start, len, c, last);
      if (r.stopped) r.status = GGRS_PACKET_STOPPED;
      if (b.live) {
        const int64_t o = (int64_t)ci * p.S + b.s;
        rows.write_outputs(k, c, o, r, last, stop);
        p.status[o] = r.status;
        p.ack[o] = last;
      }
      ci = ci + 1 == cap ? 0 : ci + 1;
    }
  }
  if (b.live) {
    p.last[b.s] = last;
    p.stop[b.s] = stop;
  }
}

}  // namespace
}  // namespace ggrs
