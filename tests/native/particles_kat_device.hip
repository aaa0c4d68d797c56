// Device harness of the particle-world KATs (tests/test_gpu_particles_kat.py): the entity step and
// the closed-form Fletcher-16 of ggrs_amd/csrc/particles.h, run on arrays the test supplies.
// Nothing is compared here: the test compares every output with the CPU oracle.  Test
// infrastructure, compiled by the test with the product's flags (step_form_cases.compile_kat).
//
// Every entry returns the first nonzero HIP error code of its allocations, copies and launches (0:
// none); the caller launches nothing more after a nonzero code.
#include "particles.h"

namespace {

using namespace ggrs;
using namespace ggrs::particles;
constexpr int kBlock = 256;  // four waves of 64 consecutive cases / entities

// device buffers of one entry, freed when it returns
struct Bufs {
  void* p[8] = {};
  int n = 0;
  hipError_t err = hipSuccess;
  ~Bufs() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  bool ok() const { return err == hipSuccess; }
  void note(hipError_t e) {
    if (err == hipSuccess) err = e;
  }
  template <typename T>
  T* alloc(size_t count) {
    if (!ok()) return nullptr;
    void* d = nullptr;
    note(hipMalloc(&d, count * sizeof(T) + 16));
    if (ok()) p[n++] = d;
    return (T*)d;
  }
  template <typename T>
  T* upload(const T* h, size_t count) {
    T* d = alloc<T>(count);
    if (ok()) note(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  // after a launch: its launch error, its execution error, then nothing if either is set
  void launched() {
    note(hipGetLastError());
    if (ok()) note(hipDeviceSynchronize());
  }
  template <typename T>
  void download(T* h, const T* d, size_t count) {
    if (ok()) note(hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost));
  }
};
inline unsigned grid_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// one advance_entity<Lean> per lane: words / out [n][25], input [n] (the byte the entity plays)
template <bool Lean>
__global__ __launch_bounds__(kBlock) void advance_kernel(int64_t n, const uint32_t* words, const uint8_t* input,
                                                          uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w[kFields];
#pragma unroll
  for (int k = 0; k < kFields; k++) w[k] = words[i * kFields + k];
  advance_entity<Lean>(w, input[i]);
#pragma unroll
  for (int k = 0; k < kFields; k++) out[i * kFields + k] = w[k];
}

// fletcher_entity_mod of every entity of `cases` records of N entities (words [cases][N][25]), with
// c_e as pw_synctest_kernel's replay_unit computes it, summed per case in plain u32:
// sums [cases][2] (zeroed by the caller) = the t1d, t2d finish_checksum takes.  blockIdx.y = case.
__global__ __launch_bounds__(kBlock) void entity_sums_kernel(int32_t N, const uint32_t* words, uint32_t* sums) {
  const int64_t c = blockIdx.y;
  const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  uint32_t s1d = 0, s2d = 0;
  if (e < N) {
    uint32_t w[kFields];
    const uint32_t* src = words + ((size_t)c * N + e) * kFields;
#pragma unroll
    for (int k = 0; k < kFields; k++) w[k] = src[k];
    const uint32_t ce = (uint32_t)(((int64_t)kEntityBytes * (N - e)) % 255);
    fletcher_entity_mod(s1d, s2d, w, ce);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s1d += (uint32_t)__shfl_xor((int)s1d, m, 64);
    s2d += (uint32_t)__shfl_xor((int)s2d, m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(sums + 2 * c, s1d);
    atomicAdd(sums + 2 * c + 1, s2d);
  }
}

// out [cases][n_frames] = finish_checksum of each case's sums with each frame counter
__global__ __launch_bounds__(kBlock) void finish_kernel(int64_t cases, int32_t n_frames, int32_t N, const uint32_t* sums,
                                                         const int32_t* frames, uint16_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cases * n_frames) return;
  const int64_t c = i / n_frames;
  out[i] = finish_checksum(sums[2 * c], sums[2 * c + 1], frames[i % n_frames], N);
}

constexpr int kBadArgument = -1;  // an argument outside the entry's forms / sizes (no HIP call made)

}  // namespace

// lean: 0 advance_entity<false> (any rotation), 1 advance_entity<true> (rotation in [+0, 2 pi])
extern "C" int kat_pw_advance(int lean, int64_t n, const uint32_t* words, const uint8_t* input, uint32_t* out) {
  if (lean < 0 || lean > 1 || n < 1) return kBadArgument;
  Bufs B;
  const uint32_t* dw = B.upload(words, (size_t)n * kFields);
  const uint8_t* din = B.upload(input, (size_t)n);
  uint32_t* dout = B.alloc<uint32_t>((size_t)n * kFields);
  if (!B.ok()) return (int)B.err;
  if (lean) advance_kernel<true><<<grid_for(n), kBlock>>>(n, dw, din, dout);
  else advance_kernel<false><<<grid_for(n), kBlock>>>(n, dw, din, dout);
  B.launched();
  B.download(out, dout, (size_t)n * kFields);
  return (int)B.err;
}

// The whole checksum of `cases` states of N entities (words [cases][N][25]) at each of n_frames
// frame counters: out [cases][n_frames].  N as the engine admits it (a multiple of 4 in 4..160000).
extern "C" int kat_pw_checksum(int64_t cases, int32_t N, int32_t n_frames, const int32_t* frames, const uint32_t* words,
                               uint16_t* out) {
  if (cases < 1 || cases > 65535 || N < 4 || N % 4 != 0 || N > 160000 || n_frames < 1) return kBadArgument;
  Bufs B;
  const uint32_t* dw = B.upload(words, (size_t)cases * N * kFields);
  const int32_t* df = B.upload(frames, (size_t)n_frames);
  uint32_t* dsums = B.alloc<uint32_t>((size_t)cases * 2);
  uint16_t* dout = B.alloc<uint16_t>((size_t)cases * n_frames);
  if (B.ok()) B.note(hipMemset(dsums, 0, (size_t)cases * 2 * sizeof(uint32_t)));
  if (!B.ok()) return (int)B.err;
  entity_sums_kernel<<<dim3(grid_for(N), (unsigned)cases), kBlock>>>(N, dw, dsums);
  B.launched();
  if (!B.ok()) return (int)B.err;
  finish_kernel<<<grid_for(cases * n_frames), kBlock>>>(cases, n_frames, N, dsums, df, dout);
  B.launched();
  B.download(out, dout, (size_t)cases * n_frames);
  return (int)B.err;
}
