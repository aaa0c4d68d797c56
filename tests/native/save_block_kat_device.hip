// Device harness of the save-block KAT (tests/test_gpu_synctest_save_block.py): the function the
// check_distance-8 SyncTest kernel's consumer wave runs per core block (synctest_save_block of
// ggrs_amd/csrc/synctest_save.h), on crafted hand-off buffers and small rings of its own.  Nothing
// is compared here: the test compares the rings and the returned lane masks with its own numpy
// restatement.  Test infrastructure, compiled by the test with the product's flags.
//
// One launch runs `blocks` one-wave blocks.  Block b has four session slots (the wave's four DPP
// rows), of which the first ctl[b].nsess exist, and an arena of its own at arena + b * stride, laid
// out as the engine's buffers for L = 4 lanes: ring [R][11][4] u32, ring_ck [R][4] u16, first_ck
// [R][4] u16 -- R * 192 bytes, which is also the buffer descriptor's size, so no store of the block
// can land outside its arena.
#include "synctest_save.h"

namespace {

using namespace ggrs;

constexpr int kSess = 4;  // session slots per block
constexpr int kBadArgument = -1;

struct BlockCtl {
  int32_t R, sr, t, nsess;
};

__global__ __launch_bounds__(kWave) void save_block_kernel(const BlockCtl* ctl, const uint32_t* hand, uint8_t* arena,
                                                           int64_t stride, unsigned long long* flagged) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_hand[kSaveHandBytes];
  const int wl = threadIdx.x;
  const int64_t b = blockIdx.x;
  const BlockCtl c = ctl[b];
  const uint32_t* src = hand + b * (kSaveHandBytes / 4);
  for (int q = wl; q < kSaveHandBytes / 4; q += kWave) reinterpret_cast<uint32_t*>(lds_hand)[q] = src[q];
  __syncthreads();
  const int g = wl / (kSaveCd * kSavePlayers), r = wl % (kSaveCd * kSavePlayers);
  const int j = r / kSavePlayers, pl = r % kSavePlayers;
  const bool valid = g < c.nsess;
  const int64_t L = kSess;
  const uint32_t ck_base = (uint32_t)(c.R * state_fields(kSavePlayers) * 4 * L);
  const uint32_t first_base = ck_base + (uint32_t)(c.R * 2 * L);
  const uint32_t bytes = first_base + (uint32_t)(c.R * 2 * L);
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(arena + b * stride, (short)0, (int)bytes, 0x00020000);
  const SaveLane lane = make_save_lane(valid, pl, g, L, ck_base, first_base);
  const uint64_t mask = synctest_save_block(lds_hand, lane, rs, c.R, (uint32_t)c.sr, c.t, wl, j, __ballot(valid));
  if (wl == 0) flagged[b] = mask;
}

}  // namespace

// ctl [blocks][4] (R, sr, t, nsess), hand [blocks][kSaveHandBytes / 4], arena [blocks][stride] (in and
// out), flagged [blocks].  Returns the first nonzero HIP error code (0: none), -1 for a bad argument.
extern "C" int kat_save_block(int blocks, const int32_t* ctl, const uint32_t* hand, uint8_t* arena, int64_t stride,
                              uint64_t* flagged) {
  if (blocks < 1 || stride < 0 || (stride & 3)) return kBadArgument;
  for (int b = 0; b < blocks; b++) {
    const int32_t R = ctl[4 * b], sr = ctl[4 * b + 1], ns = ctl[4 * b + 3];
    if (R <= kSaveCd || sr < 0 || sr >= R || ns < 0 || ns > kSess || (int64_t)R * 192 > stride) return kBadArgument;
  }
  hipError_t err = hipSuccess;
  auto note = [&](hipError_t e) {
    if (err == hipSuccess) err = e;
  };
  void *dctl = nullptr, *dhand = nullptr, *darena = nullptr, *dflag = nullptr;
  const size_t nctl = (size_t)blocks * sizeof(BlockCtl), nhand = (size_t)blocks * kSaveHandBytes;
  const size_t narena = (size_t)blocks * (size_t)stride, nflag = (size_t)blocks * 8;
  note(hipMalloc(&dctl, nctl));
  note(hipMalloc(&dhand, nhand));
  note(hipMalloc(&darena, narena + 16));
  note(hipMalloc(&dflag, nflag));
  if (err == hipSuccess) note(hipMemcpy(dctl, ctl, nctl, hipMemcpyHostToDevice));
  if (err == hipSuccess) note(hipMemcpy(dhand, hand, nhand, hipMemcpyHostToDevice));
  if (err == hipSuccess) note(hipMemcpy(darena, arena, narena, hipMemcpyHostToDevice));
  if (err == hipSuccess) {
    save_block_kernel<<<blocks, kWave>>>((const BlockCtl*)dctl, (const uint32_t*)dhand, (uint8_t*)darena, stride,
                                         (unsigned long long*)dflag);
    note(hipGetLastError());
    if (err == hipSuccess) note(hipDeviceSynchronize());
  }
  if (err == hipSuccess) note(hipMemcpy(arena, darena, narena, hipMemcpyDeviceToHost));
  if (err == hipSuccess) note(hipMemcpy(flagged, dflag, nflag, hipMemcpyDeviceToHost));
  (void)hipFree(dctl), (void)hipFree(dhand), (void)hipFree(darena), (void)hipFree(dflag);
  return (int)err;
}
