// Device harness of the increment-block KAT (tests/test_gpu_increment_block_kat.py): what the
// check_distance-8 SyncTest kernel's two waves run per core block since the block's pass publishes
// each step's velocity increment (ggrs_amd/csrc/synctest_sincos_block.h: block_rot_chain,
// increment_block_pass, increment_block_entry; box_game.h: rec_q_increment,
// advance_player_inc_turned, advance_player_inc), beside nine chained single-step calls of
// advance_player_rec_q with the hook the per-step form used.  Nothing is compared here: the test
// compares the two, bit for bit, and the states with the CPU oracle's step.  Test infrastructure,
// compiled by the test with the product's flags.
//
// advance_player_rec_q is itself rec_q_increment followed by advance_player_inc_body, so the two
// forms share that text.  What the comparison rests on beside it: ref_inc, the increment written out
// by hand below as the per-step form computed it before the split, and the chained states against
// the oracle's ship_step_batch, which shares nothing with either.
//
// One launch runs `waves` one-wave blocks.  A wave holds four sessions of 8 roles x 2 players (lane
// = session * 16 + role * 2 + player); wave b's (session, player) pair q = session * 2 + player
// starts from start[b][q] = (x, y, vx, vy, rot) and takes the inputs in[b][q][0..8]: one per step
// of the block, and the row behind it (step 0 of the next block, which role 7's entry is for) --
// every role of the pair the same, as in a core block.
#include "synctest_sincos_block.h"

namespace {

using namespace ggrs;

constexpr int kPairs = 8;            // (session, player) pairs per wave
constexpr int kRows = kSaveCd + 1;   // input rows per pair
constexpr int kBadArgument = -1;

__global__ __launch_bounds__(kWave) void increment_block_kernel(const uint32_t* start, const uint8_t* in, uint32_t* st_out,
                                                                uint32_t* r_out, uint32_t* inc_out, uint32_t* batch_out,
                                                                uint32_t* ref_st, uint32_t* ref_inc) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_hand[kSaveHandBytes];
  __shared__ __attribute__((aligned(16))) uint8_t lds_inc[kIncBlockBytes];
  const int wl = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int g = wl / (kSaveCd * kSavePlayers), r = wl % (kSaveCd * kSavePlayers);
  const int j = r / kSavePlayers, pl = r % kSavePlayers;
  const int q = g * kSavePlayers + pl;
  const uint32_t* st0 = start + (b * kPairs + q) * 5;
  InputRec rec[kRows];
#pragma unroll
  for (int u = 0; u < kRows; u++) rec[u] = make_input_rec(in[(b * kPairs + q) * kRows + u]);
  // the lane's own next-step record: row j + 1, the one its batch sub-step takes
  InputRec own = rec[1];
#pragma unroll
  for (int u = 1; u < kSaveCd; u++)
    if (j == u) own = rec[u + 1];
  const float rot0 = __builtin_bit_cast(float, st0[4]);
  const int64_t lane = b * kWave + wl;

  // the block form: the chain and the pass, then eight steps on the increment body
  {
    const InputRec turns[kSaveCd] = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]};
    float rr[kSaveCd];
    block_rot_chain(rot0, turns, rr);
    increment_block_pass(lds_hand, lds_inc, wl, j, rr, own.sgn, own.keep);
    __syncthreads();
    float x = __builtin_bit_cast(float, st0[0]), y = __builtin_bit_cast(float, st0[1]);
    float vx = __builtin_bit_cast(float, st0[2]), vy = __builtin_bit_cast(float, st0[3]);
    // step 0's increment: the evaluation in front of the loop, folded with step 0's record
    float s, c;
    uint32_t qs, qc;
    glibc_sincosf_domain_raw(rot0, &s, &c, &qs, &qc);
    VelInc inc = rec_q_increment(s, c, qs, qc, rec[0].sgn, rec[0].keep);
    float mx = 0.0f, my = 0.0f, mvx = 0.0f, mvy = 0.0f;  // the state after step j: the lane's stash
#pragma unroll
    for (int u = 0; u < kSaveCd; u++) {
      inc_out[(lane * kRows + u) * 2] = inc.ix, inc_out[(lane * kRows + u) * 2 + 1] = inc.iy;
      advance_player_inc_turned(x, y, vx, vy, inc);
      uint32_t* o = st_out + (lane * kSaveCd + u) * 4;
      o[0] = __builtin_bit_cast(uint32_t, x), o[1] = __builtin_bit_cast(uint32_t, y);
      o[2] = __builtin_bit_cast(uint32_t, vx), o[3] = __builtin_bit_cast(uint32_t, vy);
      r_out[lane * kSaveCd + u] = *reinterpret_cast<const uint32_t*>(lds_hand + u * kSaveHandSlot + kWave * 16 + wl * 4);
      if (j == u) mx = x, my = y, mvx = vx, mvy = vy;
      inc = increment_block_entry(lds_inc, wl, j, u);
    }
    // role 7's entry: step 0 of the next block
    inc_out[(lane * kRows + kSaveCd) * 2] = inc.ix, inc_out[(lane * kRows + kSaveCd) * 2 + 1] = inc.iy;
    // the consumer's batch sub-step: the state after step j, the lane's own entry, the turn from
    // its own record's (delta, thr)
    float mrot = __builtin_bit_cast(float, *reinterpret_cast<const uint32_t*>(lds_hand + j * kSaveHandSlot + kWave * 16 + wl * 4));
    advance_player_inc(mx, my, mvx, mvy, mrot, increment_block_entry(lds_inc, wl, j, j), own.delta, own.thr);
    uint32_t* o = batch_out + lane * 5;
    o[0] = __builtin_bit_cast(uint32_t, mx), o[1] = __builtin_bit_cast(uint32_t, my);
    o[2] = __builtin_bit_cast(uint32_t, mvx), o[3] = __builtin_bit_cast(uint32_t, mvy);
    o[4] = __builtin_bit_cast(uint32_t, mrot);
  }

  // the per-step form: nine chained steps, each evaluating the next step's sin/cos in its hook; the
  // increment a step adds is written out here as the per-step form computed it
  {
    float x = __builtin_bit_cast(float, st0[0]), y = __builtin_bit_cast(float, st0[1]);
    float vx = __builtin_bit_cast(float, st0[2]), vy = __builtin_bit_cast(float, st0[3]);
    float rot = rot0;
    float s, c;
    uint32_t qs, qc;
    glibc_sincosf_domain_raw(rot, &s, &c, &qs, &qc);
#pragma unroll
    for (int u = 0; u < kRows; u++) {
      const float dx = c * kMovementSpeed, dy = s * kMovementSpeed;
      const uint32_t wx = rec[u].sgn ^ (qc & rec[u].keep), wy = rec[u].sgn ^ (qs & rec[u].keep);
      ref_inc[(lane * kRows + u) * 2] = (__builtin_bit_cast(uint32_t, dx) & rec[u].keep) ^ wx;
      ref_inc[(lane * kRows + u) * 2 + 1] = (__builtin_bit_cast(uint32_t, dy) & rec[u].keep) ^ wy;
      advance_player_rec_q(x, y, vx, vy, rot, rec[u], s, c, qs, qc,
                           [&](float rn) { glibc_sincosf_domain_raw(rn, &s, &c, &qs, &qc); });
      uint32_t* o = ref_st + (lane * kRows + u) * 5;
      o[0] = __builtin_bit_cast(uint32_t, x), o[1] = __builtin_bit_cast(uint32_t, y);
      o[2] = __builtin_bit_cast(uint32_t, vx), o[3] = __builtin_bit_cast(uint32_t, vy);
      o[4] = __builtin_bit_cast(uint32_t, rot);
    }
  }
}

}  // namespace

// start [waves][8][5], in [waves][8][9]; st_out [waves][64][8][4], r_out [waves][64][8], inc_out and
// ref_inc [waves][64][9][2], batch_out [waves][64][5], ref_st [waves][64][9][5].  Returns the first
// nonzero HIP error code (0: none), -1 for a bad argument.
extern "C" int kat_increment_block(int waves, const uint32_t* start, const uint8_t* in, uint32_t* st_out, uint32_t* r_out,
                                   uint32_t* inc_out, uint32_t* batch_out, uint32_t* ref_st, uint32_t* ref_inc) {
  if (waves < 1) return kBadArgument;
  hipError_t err = hipSuccess;
  auto note = [&](hipError_t e) {
    if (err == hipSuccess) err = e;
  };
  const size_t lanes = (size_t)waves * kWave;
  const size_t nstart = (size_t)waves * kPairs * 5 * 4, nin = (size_t)waves * kPairs * kRows;
  const size_t nst = lanes * kSaveCd * 4 * 4, nr = lanes * kSaveCd * 4, ninc = lanes * kRows * 2 * 4;
  const size_t nbatch = lanes * 5 * 4, nref = lanes * kRows * 5 * 4;
  void *dstart = nullptr, *din = nullptr, *dst = nullptr, *dr = nullptr, *dinc = nullptr, *dbatch = nullptr, *dref = nullptr,
       *drinc = nullptr;
  note(hipMalloc(&dstart, nstart));
  note(hipMalloc(&din, nin));
  note(hipMalloc(&dst, nst));
  note(hipMalloc(&dr, nr));
  note(hipMalloc(&dinc, ninc));
  note(hipMalloc(&dbatch, nbatch));
  note(hipMalloc(&dref, nref));
  note(hipMalloc(&drinc, ninc));
  if (err == hipSuccess) note(hipMemcpy(dstart, start, nstart, hipMemcpyHostToDevice));
  if (err == hipSuccess) note(hipMemcpy(din, in, nin, hipMemcpyHostToDevice));
  if (err == hipSuccess) {
    increment_block_kernel<<<waves, kWave>>>((const uint32_t*)dstart, (const uint8_t*)din, (uint32_t*)dst, (uint32_t*)dr,
                                             (uint32_t*)dinc, (uint32_t*)dbatch, (uint32_t*)dref, (uint32_t*)drinc);
    note(hipGetLastError());
    if (err == hipSuccess) note(hipDeviceSynchronize());
  }
  if (err == hipSuccess) note(hipMemcpy(st_out, dst, nst, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(r_out, dr, nr, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(inc_out, dinc, ninc, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(batch_out, dbatch, nbatch, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(ref_st, dref, nref, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(ref_inc, drinc, ninc, hipMemcpyDeviceToHost));
  (void)hipFree(dstart), (void)hipFree(din), (void)hipFree(dst), (void)hipFree(dr), (void)hipFree(dinc), (void)hipFree(dbatch),
      (void)hipFree(dref), (void)hipFree(drinc);
  return (int)err;
}
