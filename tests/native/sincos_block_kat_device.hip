// Device harness of the sin/cos-block KAT (tests/test_gpu_sincos_block_kat.py): what the
// check_distance-8 SyncTest kernel's producer wave runs once per core block
// (ggrs_amd/csrc/synctest_sincos_block.h: block_rot_chain, sincos_block_pass, sincos_block_entry),
// beside eight chained single-step calls of advance_player_rec_q with the hook the per-step form
// used.  Nothing is compared here: the test compares the two, bit for bit, and the rotations with
// the CPU oracle's step.  Test infrastructure, compiled by the test with the product's flags.
//
// One launch runs `waves` one-wave blocks.  A wave holds four sessions of 8 roles x 2 players (lane
// = session * 16 + role * 2 + player); wave b's (session, player) pair q = session * 2 + player
// starts from rot0[b][q] and takes the inputs in[b][q][0..7], one per step -- every role of the pair
// the same, as in a core block.
#include "synctest_sincos_block.h"

namespace {

using namespace ggrs;

constexpr int kPairs = 8;  // (session, player) pairs per wave
constexpr int kBadArgument = -1;

__global__ __launch_bounds__(kWave) void sincos_block_kernel(const uint32_t* rot0, const uint8_t* in, uint32_t* r_out,
                                                             uint32_t* hand4, uint32_t* sc_out, uint32_t* ref_r,
                                                             uint32_t* ref_sc) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_hand[kSaveHandBytes];
  __shared__ __attribute__((aligned(16))) uint8_t lds_sc[kSincosBlockBytes];
  const int wl = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int g = wl / (kSaveCd * kSavePlayers), r = wl % (kSaveCd * kSavePlayers);
  const int j = r / kSavePlayers, pl = r % kSavePlayers;
  const int q = g * kSavePlayers + pl;
  const float start = __builtin_bit_cast(float, rot0[b * kPairs + q]);
  InputRec rec[kSaveCd];
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) rec[u] = make_input_rec(in[(b * kPairs + q) * kSaveCd + u]);

  // the block form: the chain, the pass, then what each step would read
  float rr[kSaveCd];
  block_rot_chain(start, rec, rr);
  sincos_block_pass(lds_hand, lds_sc, wl, j, rr);
  __syncthreads();
  const int64_t lane = b * kWave + wl;
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) {
    r_out[lane * kSaveCd + u] = __builtin_bit_cast(uint32_t, rr[u]);
    hand4[lane * kSaveCd + u] = *reinterpret_cast<const uint32_t*>(lds_hand + u * kSaveHandSlot + kWave * 16 + wl * 4);
    const uint4 e = sincos_block_entry(lds_sc, wl, j, u);
    uint32_t* o = sc_out + (lane * kSaveCd + u) * 4;
    o[0] = e.x, o[1] = e.y, o[2] = e.z, o[3] = e.w;
  }

  // the per-step form: eight chained steps, each evaluating the next step's sin/cos in its hook
  float x = 300.0f, y = 400.0f, vx = 0.0f, vy = 0.0f, rot = start;
  float s, c;
  uint32_t qs, qc;
  glibc_sincosf_domain_raw(rot, &s, &c, &qs, &qc);
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) {
    advance_player_rec_q(x, y, vx, vy, rot, rec[u], s, c, qs, qc,
                         [&](float rn) { glibc_sincosf_domain_raw(rn, &s, &c, &qs, &qc); });
    ref_r[lane * kSaveCd + u] = __builtin_bit_cast(uint32_t, rot);
    uint32_t* o = ref_sc + (lane * kSaveCd + u) * 4;
    o[0] = __builtin_bit_cast(uint32_t, s), o[1] = __builtin_bit_cast(uint32_t, c), o[2] = qs, o[3] = qc;
  }
}

}  // namespace

// rot0 [waves][8], in [waves][8][8]; r_out, hand4, ref_r [waves][64][8]; sc_out, ref_sc
// [waves][64][8][4].  Returns the first nonzero HIP error code (0: none), -1 for a bad argument.
extern "C" int kat_sincos_block(int waves, const uint32_t* rot0, const uint8_t* in, uint32_t* r_out, uint32_t* hand4,
                                uint32_t* sc_out, uint32_t* ref_r, uint32_t* ref_sc) {
  if (waves < 1) return kBadArgument;
  hipError_t err = hipSuccess;
  auto note = [&](hipError_t e) {
    if (err == hipSuccess) err = e;
  };
  const size_t nrot = (size_t)waves * kPairs * 4, nin = (size_t)waves * kPairs * kSaveCd;
  const size_t nr = (size_t)waves * kWave * kSaveCd * 4, nsc = nr * 4;
  void *drot = nullptr, *din = nullptr, *dr = nullptr, *dh = nullptr, *dsc = nullptr, *drr = nullptr, *drsc = nullptr;
  note(hipMalloc(&drot, nrot));
  note(hipMalloc(&din, nin));
  note(hipMalloc(&dr, nr));
  note(hipMalloc(&dh, nr));
  note(hipMalloc(&dsc, nsc));
  note(hipMalloc(&drr, nr));
  note(hipMalloc(&drsc, nsc));
  if (err == hipSuccess) note(hipMemcpy(drot, rot0, nrot, hipMemcpyHostToDevice));
  if (err == hipSuccess) note(hipMemcpy(din, in, nin, hipMemcpyHostToDevice));
  if (err == hipSuccess) {
    sincos_block_kernel<<<waves, kWave>>>((const uint32_t*)drot, (const uint8_t*)din, (uint32_t*)dr, (uint32_t*)dh,
                                          (uint32_t*)dsc, (uint32_t*)drr, (uint32_t*)drsc);
    note(hipGetLastError());
    if (err == hipSuccess) note(hipDeviceSynchronize());
  }
  if (err == hipSuccess) note(hipMemcpy(r_out, dr, nr, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(hand4, dh, nr, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(sc_out, dsc, nsc, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(ref_r, drr, nr, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(ref_sc, drsc, nsc, hipMemcpyDeviceToHost));
  (void)hipFree(drot), (void)hipFree(din), (void)hipFree(dr), (void)hipFree(dh), (void)hipFree(dsc), (void)hipFree(drr),
      (void)hipFree(drsc);
  return (int)err;
}
