// events_device.h -- a session's GgrsEvent queue on the device, shared by the two units that own one:
// p2p_events.hip (P2PSession::event_queue, src/sessions/p2p_session.rs:149) and spectator_events.hip
// (SpectatorSession's, src/sessions/p2p_spectator_session.rs:199-239).  The step is what a call pushes
// and when the queue is cut back to MAX_EVENT_QUEUE_SIZE = 100: poll_remote_clients' handle_event
// (p2p_session.rs:430-469, :846-902: every handled endpoint event ends in the trim, a handled Input
// included, which pushes nothing), then compare_local_checksums_against_peers (:904-937) and
// check_wait_recommendation (:804-817), which push without a trim -- the queue may hold more than 100
// events until the next endpoint event.  Who owns the queue is a compile-time property of the step
// (kSession): a SpectatorSession has the first part only, for its one endpoint.
//
// Collect (ev_collect_walk): one thread per session, one wave per block; the invocation's calls are
// walked in order because the queue carries from call to call.  Head, length, the drop counter, the
// status and the closing call live in registers for the launch, loaded from and stored to [fields][S]
// rows.  A group of calls' row bytes is loaded before its first use, packed into two words and an i32 a
// call; records are stored by address, one 16-byte store each.  No LDS, no scratch.  An invocation's
// desync records come as a list in no order: ev_bucket_kernel files each under its session (kEvStageD
// places, an atomic counter a session -- nothing waits), and the session's thread takes those of call c
// in ascending (frame, checksums) order, marking a taken place.
//
// Drain (ev_drain): the per-block sums of the lengths, their exclusive scan by one workgroup, and the
// scatter into one dense list -- three launches in stream order; no block waits for another block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "events_host.h"
#include "ggrs_amd.h"

namespace ggrs {

constexpr int kEvBlock = 64;  // one wave of sessions
constexpr int kEvGroup = 8;   // calls whose row bytes are loaded together, ahead of their steps
constexpr int kEvMaxK = 4;    // spectator endpoints per session, at most (p2p_spec_emit.hip)

struct EventQueue {
  int32_t head, len, dropped, status, closed_call;
};

// Where a launch's records go: the ring [cap][S] as 16-byte words, the session's column
struct EvRing {
  uint4* ring;
  int64_t S, s;
  int32_t cap;
};

static_assert(sizeof(ggrs_event_record_t) == sizeof(uint4), "a record is one 16-byte store");

// push_back; a full ring drops its oldest record (the reference's VecDeque grows)
__device__ __forceinline__ void ev_push(EventQueue& q, const EvRing& r, uint32_t kind, uint32_t endpoint, int32_t c,
                                        uint32_t lo, uint32_t hi) {
  if (q.len == r.cap) {
    q.head = q.head + 1 == r.cap ? 0 : q.head + 1;
    q.len--;
    q.dropped++;
  }
  int32_t pos = q.head + q.len;
  if (pos >= r.cap) pos -= r.cap;
  r.ring[(int64_t)pos * r.S + r.s] = make_uint4(kind | endpoint << 8, (uint32_t)c, lo, hi);
  q.len++;
}

// the end of handle_event (p2p_session.rs:898-901): the oldest go while more than 100 are queued
__device__ __forceinline__ void ev_trim(EventQueue& q, int32_t cap) {
  if (q.len > kEvMaxQueue) {
    q.head += q.len - kEvMaxQueue;
    if (q.head >= cap) q.head -= cap;
    q.len = kEvMaxQueue;
  }
}

__device__ __forceinline__ void ev_push_trim(EventQueue& q, const EvRing& r, uint32_t kind, uint32_t endpoint, int32_t c,
                                             uint64_t payload) {
  ev_push(q, r, kind, endpoint, c, (uint32_t)payload, (uint32_t)(payload >> 32));
  ev_trim(q, r.cap);
}

// One endpoint's events of call c in the fixed order Resumed, the requested Disconnected, Interrupted,
// the timeout's Disconnected.  `main` is the endpoint whose closing the queue remembers (a P2P session's
// remote endpoint, a spectator's host): a Disconnected is pushed for it while it is open only, and
// `closes` (a disconnect request, or the host's own disconnect_player) closes it without an event.
__device__ __forceinline__ void ev_endpoint_events(EventQueue& q, const EvRing& r, int32_t c, uint32_t endpoint, uint32_t net,
                                                   bool main, bool disc_req, bool closes, uint64_t interrupted_ms) {
  if (net & GGRS_NET_RESUMED) ev_push_trim(q, r, GGRS_EVENT_NETWORK_RESUMED, endpoint, c, 0);
  if (main) {
    if (disc_req && q.closed_call < 0) ev_push_trim(q, r, GGRS_EVENT_DISCONNECTED, endpoint, c, 0);
    if ((disc_req || closes) && q.closed_call < 0) q.closed_call = c;
  }
  if (net & GGRS_NET_INTERRUPTED) ev_push_trim(q, r, GGRS_EVENT_NETWORK_INTERRUPTED, endpoint, c, interrupted_ms);
  if (net & GGRS_NET_DISCONNECTED) {
    if (!main) {
      ev_push_trim(q, r, GGRS_EVENT_DISCONNECTED, endpoint, c, 0);
    } else if (q.closed_call < 0) {
      ev_push_trim(q, r, GGRS_EVENT_DISCONNECTED, endpoint, c, 0);
      q.closed_call = c;
    }
  }
}

// What a collect launch takes: S sessions, calls c0 .. c0 + n - 1; every row may be null (nothing
// happened).  A spectator engine's launch has net_events and handled only.
struct EvCollect {
  int64_t S;
  int32_t c0, n, cap;
  int32_t K;                  // spectator endpoints per session (0..kEvMaxK)
  uint32_t rmask;             // the remote players' event bits
  uint64_t interrupted_ms;    // disconnect_timeout - disconnect_notify_start of the main endpoint
  uint64_t spec_interrupted_ms;  // ... of the spectator endpoints
  const uint8_t* events;      // [n][S]
  const uint8_t* disc_req;    // [n][S]
  const uint8_t* handled;     // [n][S]
  const uint8_t* net;         // [n][S]
  const uint8_t* spec_net;    // [n][K][S]
  const int32_t* skip;        // [n][S]
  uint4* ring;                // [cap][S]
  int32_t* st;                // [kEvFields][S]
  int32_t* stage;             // [kEvStagePlanes][kEvStageD][S], or null: the invocation has no desync record
  int32_t* stage_count;       // [S]
};

// The launch loop of a collect kernel (kEvBlock threads a block, grid_of(S, kEvBlock) blocks).
template <bool kSession>
__device__ __forceinline__ void ev_collect_walk(const EvCollect& p) {
  const int64_t S = p.S;
  const int64_t s = (int64_t)blockIdx.x * kEvBlock + threadIdx.x;
  if (s >= S) return;  // (no barrier below)
  EventQueue q;
  q.head = p.st[(int64_t)kEvHead * S + s];
  q.len = p.st[(int64_t)kEvLen * S + s];
  q.dropped = p.st[(int64_t)kEvDropped * S + s];
  q.status = p.st[(int64_t)kEvStatus * S + s];
  q.closed_call = p.st[(int64_t)kEvClosedCall * S + s];
  const EvRing r{p.ring, S, s, p.cap};
  // the session's staged desync records of this invocation
  int32_t staged = 0;
  if constexpr (kSession) {
    if (p.stage) {
      const int32_t filed = p.stage_count[s];
      if (filed > kEvStageD) q.status = GGRS_EVENTS_LOST;
      staged = min(filed, kEvStageD);
      if (filed) p.stage_count[s] = 0;  // (the next invocation's bucket starts empty)
    }
  }
  const int K = kSession ? p.K : 0;

  for (int32_t k0 = 0; k0 < p.n; k0 += kEvGroup) {
    const int gn = min(kEvGroup, p.n - k0);
    // the group's row bytes, all loads in flight together (a short group repeats its last call):
    // events | disc_req << 8 | handled << 16 | net_events << 24, the spectator endpoints' net_events at
    // four bits each, skip_frames
    uint32_t w8[kEvGroup], sp8[kEvGroup];
    int32_t sk8[kEvGroup];
#pragma unroll
    for (int g = 0; g < kEvGroup; g++) {
      const int64_t k = k0 + min(g, gn - 1);
      const int64_t i = k * S + s;
      uint32_t w = p.net ? (uint32_t)p.net[i] << 24 : 0u;
      if (p.handled) w |= (uint32_t)(p.handled[i] != 0) << 16;
      uint32_t sp = 0;
      int32_t sk = 0;
      if constexpr (kSession) {
        if (p.events) w |= (uint32_t)p.events[i];
        if (p.disc_req) w |= (uint32_t)(p.disc_req[i] != 0) << 8;
        if (p.spec_net)
#pragma unroll
          for (int j = 0; j < kEvMaxK; j++)
            if (j < K) sp |= ((uint32_t)p.spec_net[(k * K + j) * S + s] & 15u) << (4 * j);
        if (p.skip) sk = p.skip[i];
      }
      w8[g] = w;
      sp8[g] = sp;
      sk8[g] = sk;
    }
    for (int g = 0; g < gn; g++) {
      const int32_t c = p.c0 + k0 + g;
      // this call's words: the front of the batch, which shifts down a call per iteration (indexing it
      // by g would put it in scratch memory)
      const uint32_t w = w8[0], sp = sp8[0];
      const int32_t sk = sk8[0];
#pragma unroll
      for (int j = 0; j < kEvGroup - 1; j++) {
        w8[j] = w8[j + 1];
        sp8[j] = sp8[j + 1];
        sk8[j] = sk8[j + 1];
      }
      // a. poll_remote_clients: the remote endpoint (the host), then the spectator endpoints in order
      ev_endpoint_events(q, r, c, 0, w >> 24, true, (w >> 8 & 1u) != 0, (w & p.rmask) != 0, p.interrupted_ms);
      if constexpr (kSession) {
        if (sp)
          for (int j = 0; j < K; j++)
            ev_endpoint_events(q, r, c, 1 + j, sp >> (4 * j) & 15u, false, false, false, p.spec_interrupted_ms);
      }
      if (w >> 16 & 1u) ev_trim(q, p.cap);  // Event::Input: handled, nothing pushed
      if constexpr (kSession) {
        // b. compare_local_checksums_against_peers: the call's records in ascending frame order, no trim
        if (staged > 0) {
          for (;;) {
            int32_t best = -1;
            uint64_t best_key = 0;
            for (int32_t i = 0; i < staged; i++) {
              if (p.stage[((int64_t)kEvStageCall * kEvStageD + i) * S + s] != c) continue;
              const uint64_t key = (uint64_t)(uint32_t)p.stage[((int64_t)kEvStageFrame * kEvStageD + i) * S + s] << 32 |
                                   (uint32_t)p.stage[((int64_t)kEvStageChecksums * kEvStageD + i) * S + s];
              if (best < 0 || key < best_key) {
                best = i;
                best_key = key;
              }
            }
            if (best < 0) break;
            p.stage[((int64_t)kEvStageCall * kEvStageD + best) * S + s] = -1;  // taken
            ev_push(q, r, GGRS_EVENT_DESYNC_DETECTED, 0, c, (uint32_t)(best_key >> 32), (uint32_t)best_key);
          }
        }
        // c. check_wait_recommendation, no trim
        if (sk > 0) ev_push(q, r, GGRS_EVENT_WAIT_RECOMMENDATION, 0, c, (uint32_t)sk, 0);
      }
    }
  }
  p.st[(int64_t)kEvHead * S + s] = q.head;
  p.st[(int64_t)kEvLen * S + s] = q.len;
  p.st[(int64_t)kEvDropped * S + s] = q.dropped;
  p.st[(int64_t)kEvStatus * S + s] = q.status;
  p.st[(int64_t)kEvClosedCall * S + s] = q.closed_call;
}

// A desync record list of m records (no order) into the sessions' staging places: the records of calls
// c0 .. c0 + n - 1 and sessions 0 .. S - 1, the others are passed over.  `words` (the engine's own list)
// holds local | remote << 16 where the caller's arrays have `local` and `remote`.
static __global__ void ev_bucket_kernel(int64_t S, int32_t c0, int32_t n, int64_t first, int64_t m, const int32_t* call,
                                        const int32_t* session, const int32_t* frame, const uint16_t* local,
                                        const uint16_t* remote, const int32_t* words, int32_t* stage, int32_t* stage_count) {
  const int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int32_t c = call[i];
  const int64_t s = session[i];
  if (c < c0 || c - c0 >= n || s < 0 || s >= S) return;
  const int32_t slot = atomicAdd(&stage_count[s], 1);
  if (slot >= kEvStageD) return;  // the session's thread sees the count and sets GGRS_EVENTS_LOST
  const uint32_t ck = words ? (uint32_t)words[i] : (uint32_t)local[i] | (uint32_t)remote[i] << 16;
  stage[((int64_t)kEvStageCall * kEvStageD + slot) * S + s] = c;
  stage[((int64_t)kEvStageFrame * kEvStageD + slot) * S + s] = frame[i];
  stage[((int64_t)kEvStageChecksums * kEvStageD + slot) * S + s] = (int32_t)ck;
}

static inline int ev_bucket(EventQueueHost& q, int32_t c0, int32_t n, int64_t first, int64_t m, const int32_t* call,
                            const int32_t* session, const int32_t* frame, const uint16_t* local, const uint16_t* remote,
                            const int32_t* words, hipStream_t stream) {
  if (m <= first) return GGRS_OK;
  ev_bucket_kernel<<<grid_of(m - first, 256), 256, 0, stream>>>((int64_t)q.S, c0, n, first, m, call, session, frame, local,
                                                                 remote, words, q.stage, q.stage_count);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

// ---- the drain

// an inclusive scan over the block's kEvScanBlock values (sh: kEvScanBlock words)
template <class T>
__device__ __forceinline__ T ev_block_scan(T v, T* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kEvScanBlock; d <<= 1) {
    const T x = t >= d ? sh[t - d] : T(0);
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  return sh[t];
}

// 1. every block's records
static __global__ __launch_bounds__(kEvScanBlock) void ev_count_kernel(const int32_t* st, int64_t S, int64_t* block_sums) {
  __shared__ int32_t sh[kEvScanBlock];
  const int64_t s = (int64_t)blockIdx.x * kEvScanBlock + threadIdx.x;
  const int32_t len = s < S ? st[(int64_t)kEvLen * S + s] : 0;
  ev_block_scan(len, sh);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = sh[kEvScanBlock - 1];
}

// 2. one workgroup: the block sums become their exclusive scan; meta = {records queued, records taken = 0}
static __global__ __launch_bounds__(kEvScanBlock) void ev_scan_blocks_kernel(int64_t* block_sums, int64_t nb,
                                                                            unsigned long long* meta) {
  __shared__ int64_t sh[kEvScanBlock];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kEvScanBlock) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < nb ? block_sums[b] : 0;
    const int64_t incl = ev_block_scan(v, sh);
    if (b < nb) block_sums[b] = carry + incl - v;
    carry += sh[kEvScanBlock - 1];
    __syncthreads();  // (sh is written again by the next chunk)
  }
  if (threadIdx.x == 0) {
    meta[0] = (unsigned long long)carry;
    meta[1] = 0;
  }
}

// 3. the sessions whose records end at or before max_records hand them over, in session order then
// queue order, and are left empty; the first session that does not fit and all after it keep theirs
static __global__ __launch_bounds__(kEvScanBlock) void ev_scatter_kernel(const uint4* ring, int32_t* st, int64_t S, int32_t cap,
                                                                        const int64_t* block_offs, int64_t max_records,
                                                                        int32_t* out_session, uint4* out_records,
                                                                        unsigned long long* meta) {
  __shared__ int32_t sh[kEvScanBlock];
  const int64_t s = (int64_t)blockIdx.x * kEvScanBlock + threadIdx.x;
  const bool live = s < S;
  const int32_t len = live ? st[(int64_t)kEvLen * S + s] : 0;
  const int32_t incl = ev_block_scan(len, sh);
  const int64_t end = block_offs[blockIdx.x] + incl;
  const bool take = live && len > 0 && end <= max_records;
  if (take) {
    int32_t pos = st[(int64_t)kEvHead * S + s];
    for (int64_t o = end - len; o < end; o++) {
      out_session[o] = (int32_t)s;
      out_records[o] = ring[(int64_t)pos * S + s];
      pos = pos + 1 == cap ? 0 : pos + 1;
    }
    st[(int64_t)kEvHead * S + s] = 0;
    st[(int64_t)kEvLen * S + s] = 0;
  }
  __syncthreads();  // (the scan's words were read)
  ev_block_scan(take ? len : 0, sh);
  if (threadIdx.x == 0 && sh[kEvScanBlock - 1] > 0) atomicAdd(&meta[1], (unsigned long long)sh[kEvScanBlock - 1]);
}

// The drain of either owner: up to max_records records into `session` and `records` (host arrays, or
// with on_device device arrays written in place), *n_read of them, *n_left still queued.  Waits for its
// launches: the two counts are the host's.
static inline int ev_drain(EventQueueHost& q, int32_t max_records, int32_t* session, ggrs_event_record_t* records,
                           int32_t* n_read, int32_t* n_left, int32_t on_device, hipStream_t stream) {
  if (max_records < 0) return set_error(GGRS_E_INVALID, "max_records must be >= 0");
  if (max_records > 0 && (!session || !records)) return set_error(GGRS_E_INVALID, "null argument");
  if (on_device && ((uintptr_t)records & 15)) return set_error(GGRS_E_INVALID, "device records must be 16-byte aligned");
  const int64_t S = (int64_t)q.S, nb = grid_of(S, kEvScanBlock);
  ev_count_kernel<<<nb, kEvScanBlock, 0, stream>>>(q.st, S, q.block_offs);
  HIP_TRY(hipGetLastError());
  ev_scan_blocks_kernel<<<1, kEvScanBlock, 0, stream>>>(q.block_offs, nb, q.meta);
  HIP_TRY(hipGetLastError());
  unsigned long long meta[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(meta, q.meta, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const size_t m = (size_t)std::min<unsigned long long>(meta[0], (unsigned long long)max_records);
  if (m > 0) {
    int32_t* d_session = session;
    uint4* d_records = reinterpret_cast<uint4*>(records);
    if (!on_device) {
      if (int rc = grow_staging(&q.staging, &q.staging_bytes, m * (sizeof(uint4) + sizeof(int32_t)))) return rc;
      d_records = reinterpret_cast<uint4*>(q.staging);
      d_session = reinterpret_cast<int32_t*>(q.staging + m * sizeof(uint4));
    }
    ev_scatter_kernel<<<nb, kEvScanBlock, 0, stream>>>(reinterpret_cast<const uint4*>(q.ring), q.st, S, q.capacity,
                                                       q.block_offs, (int64_t)max_records, d_session, d_records, q.meta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&meta[1], q.meta + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (!on_device && meta[1] > 0) {
      HIP_TRY(hipMemcpyAsync(records, d_records, (size_t)meta[1] * sizeof(uint4), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipMemcpyAsync(session, d_session, (size_t)meta[1] * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
  }
  if (n_read) *n_read = (int32_t)meta[1];
  if (n_left) *n_left = (int32_t)(meta[0] - meta[1]);
  return GGRS_OK;
}

}  // namespace ggrs
