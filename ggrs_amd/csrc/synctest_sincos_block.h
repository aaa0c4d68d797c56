// synctest_sincos_block.h -- the rotations of one 8-step core block of the check_distance-8,
// two-player SyncTest kernel (engine.hip, synctest_pipelined_v5_kernel<2, true>) and their sin/cos,
// evaluated once per block by the producer wave instead of once per step.  Also run, as it
// stands, by tests/native/sincos_block_kat_device.hip.
//
// A wave holds four sessions of 8 chain roles x 2 player lanes: lane = session * 16 + role * 2 +
// player (synctest_save.h).  In a core step every role of a session holds the same state, and a
// step's new rot depends on nothing but the old rot and the step's InputRec:
//     a = rot + delta;  rot = a + (a < 0 ? 2pi : a >= thr ? -2pi : 0)         (advance_player_rec_q)
// All eight records of a block are in registers at its head, so every lane can run the eight turns
// of the block at once (block_rot_chain): r[u] is the rot after step u's turn, the rot step u + 1
// starts from.  The sin/cos a step needs is that of the rot it starts from, so the eight values a
// block's steps 1..7 and the next block's step 0 need are the sin/cos of r[0..7]: the lane of role
// j evaluates glibc_sincosf_domain_raw(r[j]) -- one polynomial pass per block on every lane
// instead of eight -- and publishes it as one 16-byte entry (sr, cr, qs, qc) in LDS; step u + 1
// reads the entry of lane (its session, role u, its player).
//
// Why the results are what one evaluation per step gave:
//   * the turns are the two f32 operations of advance_player_rec_q, in its order, with its compare
//     forms, on the same operands (the lane's own rot at the block's head, then its own r[u - 1]):
//     r[u] is bit for bit the rot the per-step form held after step u.  The per-step form rotated
//     rot one role up after every step; with all roles equal that move changes no value.
//   * glibc_sincosf_domain_raw is called unchanged, on r[j]; the per-step form called it on the
//     same value (the hook saw r[u] before the role rotation, every role's r[u] being equal), so
//     the entry's four words are the four values step u + 1 held in registers.
//   * nothing else in the step reads rot (advance_player_rec_q_turned is the same text without the
//     turn), and field 4 of the hand-off is r[u], as before.
//   * roles that differ (which the per-step form's rotation would have carried from role to role):
//     every lane still hands over its own rot of every step, so synctest_save_block's comparison
//     raises the launch's flag exactly when some role's field differs at some step, and the host
//     replays the launch on the sequential kernel; nothing the flagged launch stored survives.
//     A lane then may have read an entry computed from another role's differing rot: only in a
//     launch that is discarded.
//
// The select of r[j] by role costs no compare/select ladder: the eight r[u] go where the hand-off's
// field-4 words of the block's eight slots go anyway, and the lane reads its own word of slot j back
// (the same lane, the same address class: the wave's LDS queue is in order).
#pragma once
#include <hip/hip_runtime.h>

#include "box_game.h"
#include "glibc_sincosf.h"
#include "synctest_save.h"

namespace ggrs {

constexpr int kSincosEntry = 16;                       // (sr, cr, qs, qc)
constexpr int kSincosBlockBytes = kWave * kSincosEntry;  // one block's entries, one per lane

// r[u]: the rot after step u's turn, from the rot at the block's head and the block's records
// (delta and thr only).
__device__ __forceinline__ void block_rot_chain(float rot0, const InputRec (&rec)[kSaveCd], float (&r)[kSaveCd]) {
  float rot = rot0;
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) {
    const float a = rot + __builtin_bit_cast(float, rec[u].delta);
    rot = a + (a < 0.0f ? kTwoPi : (a >= __builtin_bit_cast(float, rec[u].thr) ? -kTwoPi : 0.0f));
    r[u] = rot;
  }
}

// The block's pass.  hb: the block's hand-off buffer (kSaveHandBytes), whose field-4 words of all
// eight slots this writes; sc: the block's entry buffer (kSincosBlockBytes); wl, j: the lane and
// its role.  The caller orders the entry writes before other lanes' reads (one wave: a compiler
// fence and the wave's in-order LDS queue).
__device__ __forceinline__ void sincos_block_pass(uint8_t* hb, uint8_t* sc, int wl, int j, const float (&r)[kSaveCd]) {
  uint8_t* own = hb + kWave * 16 + wl * 4;  // the lane's field-4 word of slot 0
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) *reinterpret_cast<uint32_t*>(own + u * kSaveHandSlot) = __builtin_bit_cast(uint32_t, r[u]);
  const uint32_t rj = *reinterpret_cast<const uint32_t*>(own + j * kSaveHandSlot);
  float s, c;
  uint32_t qs, qc;
  glibc_sincosf_domain_raw(__builtin_bit_cast(float, rj), &s, &c, &qs, &qc);
  *reinterpret_cast<uint4*>(sc + wl * kSincosEntry) = make_uint4(__builtin_bit_cast(uint32_t, s), __builtin_bit_cast(uint32_t, c), qs, qc);
}

// What step u + 1 of the block (u = 7: step 0 of the next block) needs on lane wl of role j: the
// entry of lane (session, role u, player), one 16-byte read.
__device__ __forceinline__ uint4 sincos_block_entry(const uint8_t* sc, int wl, int j, int u) {
  return *reinterpret_cast<const uint4*>(sc + (wl + (u - j) * kSavePlayers) * kSincosEntry);
}

}  // namespace ggrs
