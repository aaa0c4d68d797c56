// Device harness of the step-form KATs (tests/test_gpu_step_forms.py): every form of the box-game
// step, the fused Fletcher-16 and the in-domain sin/cos forms of ggrs_amd/csrc/box_game.h, run one
// lane per case on arrays the test supplies.  Nothing is compared here: the test compares every
// output with the CPU oracle.  Test infrastructure, compiled by the test with the product's flags.
//
// Every entry returns the first nonzero HIP error code of its allocations, copies and launch (0:
// none); the caller launches nothing more after a nonzero code.
#include "box_game.h"

namespace {

using namespace ggrs;
constexpr int kBlock = 256;  // four waves of 64 consecutive cases

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

enum StepForm { kGeneral = 0, kDispatch, kDomain, kLean, kLeanSc, kRec, kRecQ, kStepForms };

template <int FORM>
__global__ __launch_bounds__(kBlock) void step_kernel(int64_t n, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float x = __builtin_bit_cast(float, in[5 * i + 0]), y = __builtin_bit_cast(float, in[5 * i + 1]);
  float vx = __builtin_bit_cast(float, in[5 * i + 2]), vy = __builtin_bit_cast(float, in[5 * i + 3]);
  float rot = __builtin_bit_cast(float, in[5 * i + 4]);
  const uint32_t b = input[i];
  if constexpr (FORM == kGeneral) advance_player_general(x, y, vx, vy, rot, b);
  if constexpr (FORM == kDispatch) advance_player(x, y, vx, vy, rot, b);
  if constexpr (FORM == kDomain) advance_player_domain(x, y, vx, vy, rot, b);
  if constexpr (FORM == kLean) advance_player_lean(x, y, vx, vy, rot, b);
  if constexpr (FORM == kLeanSc) {
    float s, c;
    glibc_sincosf_domain(rot, &s, &c);
    advance_player_lean_sc(x, y, vx, vy, rot, b, s, c);  // (with a hook: chain_kernel)
  }
  if constexpr (FORM == kRec) {
    float s, c;
    glibc_sincosf_domain(rot, &s, &c);
    advance_player_rec(x, y, vx, vy, rot, make_input_rec(b), s, c);
  }
  if constexpr (FORM == kRecQ) {
    float sr, cr;
    uint32_t qs, qc;
    glibc_sincosf_domain_raw(rot, &sr, &cr, &qs, &qc);
    advance_player_rec_q(x, y, vx, vy, rot, make_input_rec(b), sr, cr, qs, qc);
  }
  out[5 * i + 0] = __builtin_bit_cast(uint32_t, x);
  out[5 * i + 1] = __builtin_bit_cast(uint32_t, y);
  out[5 * i + 2] = __builtin_bit_cast(uint32_t, vx);
  out[5 * i + 3] = __builtin_bit_cast(uint32_t, vy);
  out[5 * i + 4] = __builtin_bit_cast(uint32_t, rot);
}

// N independent player steps per lane: in / out [n][N][5], input [n][N]
template <int N, bool kRecForm>
__global__ __launch_bounds__(kBlock) void players_kernel(int64_t n, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const SincosConsts K = sincos_consts_vgpr();
  uint32_t v[N][5];
#pragma unroll
  for (int k = 0; k < N; k++)
#pragma unroll
    for (int q = 0; q < 5; q++) v[k][q] = in[(i * N + k) * 5 + q];
  if constexpr (kRecForm) {
    InputRec rec[N];
#pragma unroll
    for (int k = 0; k < N; k++) rec[k] = make_input_rec(input[i * N + k]);
    advance_players_rec<N>(v, rec, K);
  } else {
    uint32_t b[N];
#pragma unroll
    for (int k = 0; k < N; k++) b[k] = input[i * N + k];
    advance_players_lean<N>(v, b, K);
  }
#pragma unroll
  for (int k = 0; k < N; k++)
#pragma unroll
    for (int q = 0; q < 5; q++) out[(i * N + k) * 5 + q] = v[k][q];
}

enum StateForm { kState = 0, kStateLean, kStateLeanK, kStateForms };

// whole states: w / out [n][1 + 5P] SoA words (box_game.h's field order), inputs [n] one byte per
// player, disconnected [n] the mask (kState only); ck [n] = fletcher16_state of the result
template <int P, int FORM>
__global__ __launch_bounds__(kBlock) void state_kernel(int64_t n, const uint32_t* w, const uint32_t* inputs,
                                                        const uint32_t* disconnected, uint32_t* out, uint16_t* ck) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  constexpr int F = state_fields(P);
  BoxState<P> s;
#pragma unroll
  for (int k = 0; k < F; k++) s.w[k] = w[i * F + k];
  if constexpr (FORM == kState) advance_state<P>(s, inputs[i], disconnected[i]);
  if constexpr (FORM == kStateLean) advance_state_lean<P>(s, inputs[i]);
  if constexpr (FORM == kStateLeanK) advance_state_lean_k<P>(s, inputs[i], sincos_consts_vgpr());
#pragma unroll
  for (int k = 0; k < F; k++) out[i * F + k] = s.w[k];
  ck[i] = fletcher16_state<P>(s);
}

// `steps` consecutive steps of one player per lane, the next step's sin/cos computed inside this
// step's hook from the rotation the hook receives: form 0 the SyncTest core's pattern
// (advance_player_rec_q + glibc_sincosf_domain_raw), form 1 the request kernels'
// (advance_player_lean_sc + glibc_sincosf_domain).  input [n][steps], out [n][steps][5].
template <int FORM>
__global__ __launch_bounds__(kBlock) void chain_kernel(int64_t n, int steps, const uint32_t* in, const uint8_t* input,
                                                        uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float x = __builtin_bit_cast(float, in[5 * i + 0]), y = __builtin_bit_cast(float, in[5 * i + 1]);
  float vx = __builtin_bit_cast(float, in[5 * i + 2]), vy = __builtin_bit_cast(float, in[5 * i + 3]);
  float rot = __builtin_bit_cast(float, in[5 * i + 4]);
  float sc_s, sc_c;
  uint32_t sc_qs = 0, sc_qc = 0;
  if constexpr (FORM == 0) glibc_sincosf_domain_raw(rot, &sc_s, &sc_c, &sc_qs, &sc_qc);
  else glibc_sincosf_domain(rot, &sc_s, &sc_c);
  for (int t = 0; t < steps; t++) {
    const uint32_t b = input[i * steps + t];
    if constexpr (FORM == 0) {
      advance_player_rec_q(x, y, vx, vy, rot, make_input_rec(b), sc_s, sc_c, sc_qs, sc_qc,
                           [&](float rn) { glibc_sincosf_domain_raw(rn, &sc_s, &sc_c, &sc_qs, &sc_qc); });
    } else {
      const float s0 = sc_s, c0 = sc_c;
      advance_player_lean_sc(x, y, vx, vy, rot, b, s0, c0, [&](float rn) { glibc_sincosf_domain(rn, &sc_s, &sc_c); });
    }
    uint32_t* o = out + (i * steps + t) * 5;
    o[0] = __builtin_bit_cast(uint32_t, x);
    o[1] = __builtin_bit_cast(uint32_t, y);
    o[2] = __builtin_bit_cast(uint32_t, vx);
    o[3] = __builtin_bit_cast(uint32_t, vy);
    o[4] = __builtin_bit_cast(uint32_t, rot);
  }
}

// fletcher16_state<P> of arbitrary words [n][1 + 5P], and fletcher_from_doubled<kMad24> over the same
// doubled sums accumulated plainly (one byte at a time): out_state [n], out_doubled [n]
template <int P, bool kMad24>
__global__ __launch_bounds__(kBlock) void fletcher_kernel(int64_t n, const uint32_t* words, uint16_t* out_state,
                                                           uint16_t* out_doubled) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  constexpr int F = state_fields(P), nb = Fletcher<P>::n;
  BoxState<P> s;
#pragma unroll
  for (int k = 0; k < F; k++) s.w[k] = words[i * F + k];
  out_state[i] = fletcher16_state<P>(s);
  uint32_t d1 = 2u * Fletcher<P>::kSum1Const, d2 = 2u * Fletcher<P>::kSum2Const;
  for (int k = 0; k < F; k++) {
    const int o = fld_offset(P, k);
    for (int b = 0; b < 4; b++) {
      const uint32_t byte = (s.w[k] >> (8 * b)) & 0xffu;
      d1 += 2u * byte;
      d2 += 2u * byte * (uint32_t)(nb - o - b);
    }
  }
  out_doubled[i] = (uint16_t)fletcher_from_doubled<kMad24>(d1, d2);
}

__device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the sin/cos digest of sincosf_kat_device.hip's digest_kernel (the same mix, so the same golden
// value) over the four in-domain forms: 0 _domain, 1 _domain_k, 2 _domain_raw, 3 _domain_raw_k;
// the raw forms' signs are applied as bits ^ q
template <int FORM>
__global__ __launch_bounds__(kBlock) void domain_digest_kernel(uint32_t lo, uint32_t hi, unsigned long long* acc) {
  const SincosConsts K = sincos_consts_vgpr();
  uint64_t local = 0;
  for (uint64_t u = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u <= hi;
       u += (uint64_t)gridDim.x * blockDim.x) {
    const float f = __builtin_bit_cast(float, (uint32_t)u);
    uint32_t sb, cb;
    if constexpr (FORM < 2) {
      float s, c;
      if constexpr (FORM == 0) glibc_sincosf_domain(f, &s, &c);
      else glibc_sincosf_domain_k(f, &s, &c, K);
      sb = __builtin_bit_cast(uint32_t, s);
      cb = __builtin_bit_cast(uint32_t, c);
    } else {
      float sr, cr;
      uint32_t qs, qc;
      if constexpr (FORM == 2) glibc_sincosf_domain_raw(f, &sr, &cr, &qs, &qc);
      else glibc_sincosf_domain_raw_k(f, &sr, &cr, &qs, &qc, K);
      sb = __builtin_bit_cast(uint32_t, sr) ^ qs;
      cb = __builtin_bit_cast(uint32_t, cr) ^ qc;
    }
    local += mix64((u << 32) | sb) + mix64(((u << 32) | cb) ^ 0xC05C05C05C05C05Cull);
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(acc, (unsigned long long)local);
}

// sincos_consts_vgpr() as the device materialises it (ten doubles, SincosConsts's field order)
__global__ void consts_kernel(double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const SincosConsts K = sincos_consts_vgpr();
  const double v[10] = {K.hpi_inv24, K.magic, K.hpi, K.s1, K.s2, K.s3, K.c1, K.c2, K.c3, K.c4};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}

template <int N>
void launch_players(int form, int64_t n, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  if (form == 0) players_kernel<N, false><<<grid_for(n), kBlock>>>(n, in, input, out);
  else players_kernel<N, true><<<grid_for(n), kBlock>>>(n, in, input, out);
}
template <int P>
void launch_state(int form, int64_t n, const uint32_t* w, const uint32_t* in, const uint32_t* disc, uint32_t* out,
                  uint16_t* ck) {
  if (form == kState) state_kernel<P, kState><<<grid_for(n), kBlock>>>(n, w, in, disc, out, ck);
  else if (form == kStateLean) state_kernel<P, kStateLean><<<grid_for(n), kBlock>>>(n, w, in, disc, out, ck);
  else state_kernel<P, kStateLeanK><<<grid_for(n), kBlock>>>(n, w, in, disc, out, ck);
}
template <int P>
void launch_fletcher(int mad24, int64_t n, const uint32_t* words, uint16_t* a, uint16_t* b) {
  if (mad24) fletcher_kernel<P, true><<<grid_for(n), kBlock>>>(n, words, a, b);
  else fletcher_kernel<P, false><<<grid_for(n), kBlock>>>(n, words, a, b);
}
template <int P>
void fletcher_host(int64_t n, const uint32_t* words, uint16_t* out) {
  for (int64_t i = 0; i < n; i++) out[i] = fletcher16_state_host<P>(words + i * state_fields(P));
}

constexpr int kBadArgument = -1;  // an argument outside the entry's forms / sizes (no HIP call made)

}  // namespace

// the largest N of advance_players_rec<N> the product instantiates: branch.hip's NS = NK + NT with
// eight pipeline stages (kPipeMaxW) and the four trunk players
extern "C" int kat_max_players(void) { return 12; }

// form: 0 general, 1 dispatch (advance_player), 2 domain, 3 lean, 4 lean_sc (+ hook), 5 rec, 6 rec_q
extern "C" int kat_step(int form, int64_t n, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  if (form < 0 || form >= kStepForms || n < 1) return kBadArgument;
  Bufs B;
  const uint32_t* din = B.upload(in, (size_t)n * 5);
  const uint8_t* dinput = B.upload(input, (size_t)n);
  uint32_t* dout = B.alloc<uint32_t>((size_t)n * 5);
  if (!B.ok()) return (int)B.err;
  switch (form) {
    case kGeneral: step_kernel<kGeneral><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    case kDispatch: step_kernel<kDispatch><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    case kDomain: step_kernel<kDomain><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    case kLean: step_kernel<kLean><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    case kLeanSc: step_kernel<kLeanSc><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    case kRec: step_kernel<kRec><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
    default: step_kernel<kRecQ><<<grid_for(n), kBlock>>>(n, din, dinput, dout); break;
  }
  B.launched();
  B.download(out, dout, (size_t)n * 5);
  return (int)B.err;
}

// form: 0 advance_players_lean<N>, 1 advance_players_rec<N>; N in {1, 2, 4, kat_max_players()}
extern "C" int kat_players(int form, int N, int64_t n, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  if (form < 0 || form > 1 || n < 1 || !(N == 1 || N == 2 || N == 4 || N == 12)) return kBadArgument;
  Bufs B;
  const uint32_t* din = B.upload(in, (size_t)n * N * 5);
  const uint8_t* dinput = B.upload(input, (size_t)n * N);
  uint32_t* dout = B.alloc<uint32_t>((size_t)n * N * 5);
  if (!B.ok()) return (int)B.err;
  if (N == 1) launch_players<1>(form, n, din, dinput, dout);
  else if (N == 2) launch_players<2>(form, n, din, dinput, dout);
  else if (N == 4) launch_players<4>(form, n, din, dinput, dout);
  else launch_players<12>(form, n, din, dinput, dout);
  B.launched();
  B.download(out, dout, (size_t)n * N * 5);
  return (int)B.err;
}

// form: 0 advance_state<P> (with the disconnected mask), 1 advance_state_lean<P>, 2 advance_state_lean_k<P>
extern "C" int kat_state(int form, int P, int64_t n, const uint32_t* w, const uint32_t* inputs,
                         const uint32_t* disconnected, uint32_t* out, uint16_t* ck) {
  if (form < 0 || form >= kStateForms || P < 1 || P > 4 || n < 1) return kBadArgument;
  const size_t F = 1 + 5 * (size_t)P;
  Bufs B;
  const uint32_t* dw = B.upload(w, (size_t)n * F);
  const uint32_t* din = B.upload(inputs, (size_t)n);
  const uint32_t* ddisc = B.upload(disconnected, (size_t)n);
  uint32_t* dout = B.alloc<uint32_t>((size_t)n * F);
  uint16_t* dck = B.alloc<uint16_t>((size_t)n);
  if (!B.ok()) return (int)B.err;
  if (P == 1) launch_state<1>(form, n, dw, din, ddisc, dout, dck);
  else if (P == 2) launch_state<2>(form, n, dw, din, ddisc, dout, dck);
  else if (P == 3) launch_state<3>(form, n, dw, din, ddisc, dout, dck);
  else launch_state<4>(form, n, dw, din, ddisc, dout, dck);
  B.launched();
  B.download(out, dout, (size_t)n * F);
  B.download(ck, dck, (size_t)n);
  return (int)B.err;
}

// form: 0 rec_q + domain_raw in the hook, 1 lean_sc + domain in the hook
extern "C" int kat_chain(int form, int64_t n, int steps, const uint32_t* in, const uint8_t* input, uint32_t* out) {
  if (form < 0 || form > 1 || n < 1 || steps < 1 || steps > 64) return kBadArgument;
  Bufs B;
  const uint32_t* din = B.upload(in, (size_t)n * 5);
  const uint8_t* dinput = B.upload(input, (size_t)n * steps);
  uint32_t* dout = B.alloc<uint32_t>((size_t)n * steps * 5);
  if (!B.ok()) return (int)B.err;
  if (form == 0) chain_kernel<0><<<grid_for(n), kBlock>>>(n, steps, din, dinput, dout);
  else chain_kernel<1><<<grid_for(n), kBlock>>>(n, steps, din, dinput, dout);
  B.launched();
  B.download(out, dout, (size_t)n * steps * 5);
  return (int)B.err;
}

// words [n][1 + 5P]; out_state = fletcher16_state<P>, out_doubled = fletcher_from_doubled<kMad24> of
// the plainly accumulated doubled sums, out_host = fletcher16_state_host<P> (computed on the host)
extern "C" int kat_fletcher(int P, int mad24, int64_t n, const uint32_t* words, uint16_t* out_state,
                            uint16_t* out_doubled, uint16_t* out_host) {
  if (P < 1 || P > 4 || n < 1) return kBadArgument;
  const size_t F = 1 + 5 * (size_t)P;
  if (P == 1) fletcher_host<1>(n, words, out_host);
  else if (P == 2) fletcher_host<2>(n, words, out_host);
  else if (P == 3) fletcher_host<3>(n, words, out_host);
  else fletcher_host<4>(n, words, out_host);
  Bufs B;
  const uint32_t* dw = B.upload(words, (size_t)n * F);
  uint16_t* da = B.alloc<uint16_t>((size_t)n);
  uint16_t* db = B.alloc<uint16_t>((size_t)n);
  if (!B.ok()) return (int)B.err;
  if (P == 1) launch_fletcher<1>(mad24, n, dw, da, db);
  else if (P == 2) launch_fletcher<2>(mad24, n, dw, da, db);
  else if (P == 3) launch_fletcher<3>(mad24, n, dw, da, db);
  else launch_fletcher<4>(mad24, n, dw, da, db);
  B.launched();
  B.download(out_state, da, (size_t)n);
  B.download(out_doubled, db, (size_t)n);
  return (int)B.err;
}

// the sin/cos constants the _k / raw forms read: kSincosLiteral (host) and sincos_consts_vgpr() (device),
// ten doubles each in SincosConsts's field order
extern "C" int kat_sincos_consts(double* literal, double* vgpr) {
  const SincosConsts& L = kSincosLiteral;
  const double v[10] = {L.hpi_inv24, L.magic, L.hpi, L.s1, L.s2, L.s3, L.c1, L.c2, L.c3, L.c4};
  for (int i = 0; i < 10; i++) literal[i] = v[i];
  Bufs B;
  double* d = B.alloc<double>(10);
  if (!B.ok()) return (int)B.err;
  consts_kernel<<<1, 64>>>(d);
  B.launched();
  B.download(vgpr, d, 10);
  return (int)B.err;
}

// form: 0 glibc_sincosf_domain, 1 _domain_k, 2 _domain_raw, 3 _domain_raw_k, over bits lo .. hi
extern "C" int kat_domain_digest(int form, uint32_t lo, uint32_t hi, uint64_t* out) {
  if (form < 0 || form > 3 || hi < lo) return kBadArgument;
  Bufs B;
  unsigned long long* d = B.alloc<unsigned long long>(1);
  if (B.ok()) B.note(hipMemset(d, 0, 8));
  if (!B.ok()) return (int)B.err;
  const unsigned grid = 256 * 32;
  if (form == 0) domain_digest_kernel<0><<<grid, kBlock>>>(lo, hi, d);
  else if (form == 1) domain_digest_kernel<1><<<grid, kBlock>>>(lo, hi, d);
  else if (form == 2) domain_digest_kernel<2><<<grid, kBlock>>>(lo, hi, d);
  else domain_digest_kernel<3><<<grid, kBlock>>>(lo, hi, d);
  B.launched();
  B.download((unsigned long long*)out, d, 1);
  return (int)B.err;
}
