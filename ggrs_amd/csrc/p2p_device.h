// p2p_device.h -- device routines shared by the P2P kernels of p2p.hip (fixed latency) and
// p2p_sched.hip (arrival schedules): a ring cell's packing, the copy of a block's rings between HBM
// and LDS, the staging of input rows, the InputQueue words, and the few one-liners every form had
// copied from the one before it.  The kernels keep their call logic; what is here is its plumbing.
//
// A ring cell is cell_dwords(P) / 4 pieces of 16 bytes: the state's F = state_fields(P) dwords,
// the Fletcher-16 handed to GameStateCell::save in dword F, zero padding after it.  In HBM a
// session's cells are contiguous ([S][R][pieces], p2p.hip's layout); in LDS the block's B sessions
// are the columns ([R][pieces][B]: a save is conflict-free ds_write_b128).  Every helper takes the
// cell's first piece and the piece stride B (1 in HBM) and is inlined into its caller, where an LDS
// cell is addressed from the kernel's __shared__ array itself, so its accesses stay LDS accesses (a
// pointer variable into dynamic LDS that a lambda captures becomes a generic pointer, which this
// hipcc miscompiles: p2p_sched.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "p2p_plan.h"

namespace ggrs {
namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;  // NULL_FRAME (src/lib.rs:44)
constexpr int kHist = 32;                   // MAX_CHECKSUM_HISTORY_SIZE (protocol.rs:27)

// ---- ring cells

// LoadGameState: the cell's state dwords
template <int P, int B>
__device__ __forceinline__ void cell_unpack(BoxState<P>& s, const uint4* c) {
  constexpr int F = state_fields(P);
#pragma unroll
  for (int k = 0; k < cell_dwords(P) / 4; k++) {
    const uint4 v = c[k * B];
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (4 * k + i < F) s.w[4 * k + i] = x[i];
  }
}
// SaveGameState: the state, its checksum and the padding, whole pieces
template <int P, int B>
__device__ __forceinline__ void cell_pack(const BoxState<P>& s, uint32_t ck, uint4* c) {
  constexpr int F = state_fields(P);
#pragma unroll
  for (int k = 0; k < cell_dwords(P) / 4; k++) {
    uint32_t x[4];
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = 4 * k + i < F ? s.w[4 * k + i] : (4 * k + i == F ? ck : 0u);
    c[k * B] = make_uint4(x[0], x[1], x[2], x[3]);
  }
}
// the checksum saved with the cell (the piece that holds dword F)
template <int P, int B>
__device__ __forceinline__ uint16_t cell_checksum(const uint4* c) {
  constexpr int F = state_fields(P);
  const uint4 v = c[(F / 4) * B];
  const uint32_t x[4] = {v.x, v.y, v.z, v.w};
  return (uint16_t)x[F % 4];
}

// The rings of a block's nb sessions between HBM (`hbm`: the block's first piece; its sessions'
// pieces are contiguous, so the HBM side is coalesced) and LDS columns, by every thread of the block:
// kThreads of them, or (0) blockDim.x, read where the loop steps as the kernels' own loops read it
// (whether passing it as an argument would cost a register was not measured).
// kUnroll: the copy-in's loads in flight per thread (the flat forms ask for 4), or (0) no request,
// which leaves the loop to the compiler as the scheduled kernels' own loops were.
template <int kThreads>
__device__ __forceinline__ void next_piece(int& i) {
  if constexpr (kThreads > 0) i += kThreads;
  else i += blockDim.x;
}
// HBM piece i of the block's rings in LDS: session i / ring_pieces is the column
template <int B>
__device__ __forceinline__ int lds_piece(int i, int ring_pieces) {
  const int sl = i / ring_pieces, rem = i - sl * ring_pieces;
  return rem * B + sl;
}
template <int B, int kThreads, int kUnroll = 0>
__device__ __forceinline__ void ring_to_lds(uint4* lds, const uint4* hbm, int nb, int ring_pieces) {
  const int n = nb * ring_pieces;
  if constexpr (kUnroll > 0) {
#pragma unroll kUnroll
    for (int i = threadIdx.x; i < n; next_piece<kThreads>(i)) lds[lds_piece<B>(i, ring_pieces)] = hbm[i];
  } else {
    for (int i = threadIdx.x; i < n; next_piece<kThreads>(i)) lds[lds_piece<B>(i, ring_pieces)] = hbm[i];
  }
}
template <int B, int kThreads>
__device__ __forceinline__ void ring_from_lds(uint4* hbm, const uint4* lds, int nb, int ring_pieces) {
  const int n = nb * ring_pieces;
  for (int i = threadIdx.x; i < n; next_piece<kThreads>(i)) hbm[i] = lds[lds_piece<B>(i, ring_pieces)];
}

__device__ __forceinline__ int32_t next_slot(int32_t x, int32_t R) { return x + 1 == R ? 0 : x + 1; }
__device__ __forceinline__ int32_t back_slot(int32_t x, int32_t d, int32_t R) {
  const int32_t y = x - d;
  return y < 0 ? y + R : y;
}

// ---- input rows

// byte masks of the local and the remote players' inputs in a packed row
struct ByteMasks {
  uint32_t lbytes, rbytes;
};
template <int P>
__device__ __forceinline__ ByteMasks input_byte_masks(uint32_t lmask) {
  uint32_t lbytes = 0;
#pragma unroll
  for (int k = 0; k < P; k++) lbytes |= ((lmask >> k) & 1u) ? 0xffu << (8 * k) : 0u;
  return {lbytes, (P == 4 ? 0xffffffffu : ((1u << (8 * P)) - 1u)) & ~lbytes};
}

// One stage of a one-wave block's calls [fs, end): the input rows [lo, end) of the block's nb
// sessions (from sess0) into LDS, [kRows][B][Pp] -- a call reads rows back to `back` frames behind
// it, so a stage is kRows - back calls (>= 1: the host) -- as 16-byte pieces, every load in flight,
// where the block is full and its rows are 16-byte aligned, byte by byte otherwise.  Every thread of
// the block calls it with its index `lt`; it is done with the previous stage's rows on entry and has
// these on return.
struct RowStage {
  int32_t lo, end;
};
template <int Pp, int B, int kRows>
__device__ __forceinline__ RowStage stage_rows(uint8_t* lds_rows, const uint8_t* inputs, int64_t S, int32_t cap,
                                               int64_t sess0, int nb, int lt, int32_t fs, int32_t f_end, int32_t back) {
  const int32_t calls_per_stage = kRows - back;
  const int32_t chunk_end = min(f_end, fs + calls_per_stage);
  const int32_t lo = max(0, fs - back);
  __syncthreads();
  const int nrows = chunk_end - lo, row_bytes = nb * Pp;
  if (nb == B && ((S * Pp) & 15) == 0) {
    constexpr int kPieces = B * Pp / 16;
#pragma unroll 4
    for (int c = lt; c < nrows * kPieces; c += B) {
      const int r = c / kPieces, k = c - r * kPieces;
      const uint4* src = reinterpret_cast<const uint4*>(inputs + ((int64_t)((lo + r) % cap) * S + sess0) * Pp);
      reinterpret_cast<uint4*>(lds_rows + r * B * Pp)[k] = src[k];
    }
  } else {
    for (int c = lt; c < nrows * row_bytes; c += B) {
      const int r = c / row_bytes, b = c - r * row_bytes;
      lds_rows[r * B * Pp + b] = inputs[((int64_t)((lo + r) % cap) * S + sess0) * Pp + b];
    }
  }
  __syncthreads();
  return {lo, chunk_end};
}

// ---- the remote players' InputQueues (HBM: queue [4][P][S] i32)

// The per-session state of every remote player's InputQueue that the P2P program reads.
template <int P>
struct RemoteQueues {
  int32_t pred_frame[P];  // prediction.frame (NULL: not predicting)
  uint32_t pred_in[P];    // prediction.input
  int32_t first_inc[P];   // first_incorrect_frame
  int32_t last_req[P];    // last_requested_frame
};
template <int P>
__device__ __forceinline__ void load_queues(RemoteQueues<P>& q, const int32_t* queue, int64_t S, int64_t sess) {
#pragma unroll
  for (int k = 0; k < P; k++) {
    q.pred_frame[k] = queue[(0 * P + k) * S + sess];
    q.pred_in[k] = (uint32_t)queue[(1 * P + k) * S + sess];
    q.first_inc[k] = queue[(2 * P + k) * S + sess];
    q.last_req[k] = queue[(3 * P + k) * S + sess];
  }
}
template <int P>
__device__ __forceinline__ void store_queues(const RemoteQueues<P>& q, int32_t* queue, int64_t S, int64_t sess) {
#pragma unroll
  for (int k = 0; k < P; k++) {
    queue[(0 * P + k) * S + sess] = q.pred_frame[k];
    queue[(1 * P + k) * S + sess] = (int32_t)q.pred_in[k];
    queue[(2 * P + k) * S + sess] = q.first_inc[k];
    queue[(3 * P + k) * S + sess] = q.last_req[k];
  }
}
// The remote queues after call t_last in their canonical form (the remote input of frame g arrives at
// call g + D): predicting from frame t_last - D + 1 with the input of frame t_last - D (`last_rem`,
// that frame's packed remote bytes; PredictDefault: 0), no incorrect frame, last request = the call's
// own frame.
template <int P>
__device__ __forceinline__ void store_canonical_queues(int32_t* queue, int64_t S, int64_t sess, uint32_t lmask,
                                                       int32_t t_last, int32_t D, int32_t predictor, uint32_t last_rem) {
#pragma unroll
  for (int k = 0; k < P; k++) {
    if ((lmask >> k) & 1u) continue;
    queue[(0 * P + k) * S + sess] = t_last - D + 1;
    queue[(1 * P + k) * S + sess] = (int32_t)(predictor == 0 ? (last_rem >> (8 * k)) & 0xffu : 0u);
    queue[(2 * P + k) * S + sess] = kNull;
    queue[(3 * P + k) * S + sess] = t_last;
  }
}

// ---- desync detection

// check_checksum_send_interval (p2p_session.rs:939-975) of call f, before any rollback of the call:
// last_confirmed_frame = f - 1 - D and last_saved_frame = f - 1 here, so frame_to_send = interval,
// 2 interval, ... goes out at call frame_to_send + D + 1; its cell is in the ring (D + 1 < R), its
// checksum -- cell_ck(slot) -- enters the local history ([kHist][S] u16)
template <typename CellCk>
__device__ __forceinline__ void store_desync_history(uint16_t* hist, int32_t interval, int32_t f, int32_t D, int32_t R,
                                                     int64_t S, int64_t sess, bool live, const CellCk& cell_ck) {
  if (interval > 0) {
    const int32_t fts = f - 1 - D;
    if (live && fts >= interval && fts % interval == 0)
      hist[(int64_t)((fts / interval) % kHist) * S + sess] = cell_ck(fts % R);
  }
}

}  // namespace
}  // namespace ggrs
