// poll_host.h -- the host side of an endpoint poll unit (poll_device.h has the step and the launch
// loop): the layout of the endpoints' rows kept between launches, and PollHost, what the spectator
// engine's unit (spectator_poll.hip) and the P2P engine's spectator-endpoint unit (p2p_spec_poll.hip)
// keep beside them -- the configuration, the next call, the two-slot device clock, the staging of
// host-sourced calls and the state read-back.  (p2p_poll.hip, the first of the three, keeps the same
// words as endp_* in the P2P engine object.)  Host code and plain structs only; no kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace ggrs {

// the endpoints' times and words kept between launches, [fields][E] rows over E endpoints
enum PollTime : int {
  kPollLastRecv = 0,   // last_recv_time
  kPollLastInputRecv,  // running_last_input_recv
  kPollLastReport,     // running_last_quality_report
  kPollShutdown,       // shutdown_timeout
  kPollTimes
};
enum PollField : int {
  kPollWord = 0,     // notify_sent | event_sent << 1 | state << 2 (poll_device.h)
  kPollClosedCall,   // the call at which the endpoint went Running -> Disconnected, or (an endpoint that
                     // never leaves Running: the spectator's) at which its one Disconnected was raised (-1)
  kPollFields
};
constexpr int kPollWordStateShift = 2;

struct PollHost {
  int32_t on = 0;               // the mode
  int32_t next = 0;             // the next call to poll
  int32_t launches = 0;         // launch i reads clock[i & 1] and writes clock[(i + 1) & 1]
  uint64_t timeout = 0, notify = 0;  // disconnect_timeout, disconnect_notify_start (ms)
  uint64_t host_clock = 0;      // the last clock a host array gave (a host array never goes below it)
  size_t E = 0;                 // endpoints
  uint64_t* times = nullptr;    // [kPollTimes][E]
  int32_t* st = nullptr;        // [kPollFields][E]
  uint64_t* clock = nullptr;    // [2] the engine's last clock
  uint8_t* staging = nullptr;   // host-sourced calls: the clocks, the input bytes and the outputs
  size_t staging_bytes = 0;

  void release() {
    void* bufs[] = {times, st, clock, staging};
    for (void* b : bufs)
      if (b) (void)hipFree(b);
    times = clock = nullptr;
    st = nullptr;
    staging = nullptr;
    staging_bytes = 0;
    on = 0;
    E = 0;
  }
  // Every Instant of UdpProtocol::new (protocol.rs:219-220, :252) is start_ms, and so is shutdown_timeout
  // (:227); Running, neither flag set, never closed.
  int configure(size_t endpoints, uint64_t timeout_ms, uint64_t notify_ms, uint64_t start_ms, hipStream_t stream) {
    if (notify_ms > timeout_ms)
      return set_error(GGRS_E_INVALID, "disconnect_notify_start (%llu ms) must not exceed disconnect_timeout (%llu ms)",
                       (unsigned long long)notify_ms, (unsigned long long)timeout_ms);
    if (E != endpoints) {
      uint8_t* keep = staging;  // (the staging buffer does not depend on the shape)
      const size_t keep_bytes = staging_bytes;
      staging = nullptr;
      release();
      staging = keep;
      staging_bytes = keep_bytes;
    }
    // (each buffer on its own: one that failed to allocate is the only one a later call allocates)
    if (!times) HIP_TRY(hipMalloc(&times, sizeof(uint64_t) * (size_t)kPollTimes * endpoints));
    if (!st) HIP_TRY(hipMalloc(&st, sizeof(int32_t) * (size_t)kPollFields * endpoints));
    if (!clock) HIP_TRY(hipMalloc(&clock, sizeof(uint64_t) * 2));
    E = endpoints;
    const std::vector<uint64_t> t0((size_t)kPollTimes * endpoints, start_ms);
    std::vector<int32_t> w0((size_t)kPollFields * endpoints, 0);
    for (size_t i = 0; i < endpoints; i++) w0[(size_t)kPollClosedCall * endpoints + i] = -1;
    HIP_TRY(hipMemcpyAsync(times, t0.data(), sizeof(uint64_t) * t0.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(st, w0.data(), sizeof(int32_t) * w0.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(clock, t0.data(), sizeof(uint64_t) * 2, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    on = 1;
    next = 0;
    launches = 0;
    timeout = timeout_ms;
    notify = notify_ms;
    host_clock = start_ms;
    return GGRS_OK;
  }
  // Calls first_call .. first_call + n - 1: in order, each once; a host clock never decreases.
  int check_calls(int32_t first_call, int32_t n, const uint64_t* now_ms, int32_t on_device) const {
    if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
    if (first_call != next)
      return set_error(GGRS_E_INVALID, "endpoints are polled in call order, each call once (expected call %d, got %d)", next,
                       first_call);
    if (n == 0) return GGRS_OK;
    if (!now_ms) return set_error(GGRS_E_INVALID, "null argument");
    if (!on_device) {
      uint64_t last = host_clock;
      for (int32_t k = 0; k < n; k++) {
        if (now_ms[k] < last)
          return set_error(GGRS_E_INVALID, "now_ms must not decrease (call %d: %llu after %llu)", first_call + k,
                           (unsigned long long)now_ms[k], (unsigned long long)last);
        last = now_ms[k];
      }
    }
    return GGRS_OK;
  }
  // The arrays of a launch of n calls: now_ms [n], two input byte arrays and four output byte arrays of
  // [n][E] each (any may be null).  Host arrays are staged, [now_ms][in0][in1][out0..3] (stream order
  // keeps an earlier launch's use of the buffer ahead of the copies); device arrays are used in place.
  struct Io {
    const uint64_t* now;
    const uint8_t* in[2];
    uint8_t* out[4];
  };
  int begin(const Io& host, size_t n, int32_t on_device, hipStream_t stream, Io* dev) {
    *dev = host;
    if (on_device) return GGRS_OK;
    const size_t rows = n * E, now_bytes = sizeof(uint64_t) * n;
    if (int rc = grow_staging(&staging, &staging_bytes, now_bytes + 6 * rows)) return rc;
    uint8_t* base = staging + now_bytes;
    HIP_TRY(hipMemcpyAsync(staging, host.now, now_bytes, hipMemcpyHostToDevice, stream));
    dev->now = reinterpret_cast<const uint64_t*>(staging);
    for (int i = 0; i < 2; i++)
      if (host.in[i]) {
        HIP_TRY(hipMemcpyAsync(base + (size_t)i * rows, host.in[i], rows, hipMemcpyHostToDevice, stream));
        dev->in[i] = base + (size_t)i * rows;
      }
    for (int i = 0; i < 4; i++)
      if (host.out[i]) dev->out[i] = base + (size_t)(i + 2) * rows;
    return GGRS_OK;
  }
  // ... and after the launch: the staged outputs back, waited for; the call counted
  int end(const Io& host, const Io& dev, int32_t first_call, size_t n, int32_t on_device, hipStream_t stream) {
    launches++;
    if (!on_device) {
      for (int i = 0; i < 4; i++)
        if (host.out[i]) HIP_TRY(hipMemcpyAsync(host.out[i], dev.out[i], n * E, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));  // (the host's inputs were read by then, too)
      host_clock = host.now[n - 1];
    }
    next = first_call + (int32_t)n;
    return GGRS_OK;
  }
  const uint64_t* clock_in() const { return clock + (launches & 1); }
  uint64_t* clock_out() const { return clock + ((launches & 1) ^ 1); }
  // The endpoints' state, [E] each, any may be null
  int read(int32_t* state, uint64_t* last_recv_ms, uint64_t* last_input_recv_ms, uint64_t* last_report_ms,
           uint64_t* shutdown_ms, int32_t* flags, int32_t* closed_call, hipStream_t stream) const {
    uint64_t* const dst[kPollTimes] = {last_recv_ms, last_input_recv_ms, last_report_ms, shutdown_ms};
    for (int f = 0; f < kPollTimes; f++)
      if (dst[f]) HIP_TRY(hipMemcpyAsync(dst[f], times + (size_t)f * E, sizeof(uint64_t) * E, hipMemcpyDeviceToHost, stream));
    if (closed_call)
      HIP_TRY(hipMemcpyAsync(closed_call, st + (size_t)kPollClosedCall * E, sizeof(int32_t) * E, hipMemcpyDeviceToHost, stream));
    std::vector<int32_t> word;
    if (state || flags) {
      word.resize(E);
      HIP_TRY(hipMemcpyAsync(word.data(), st + (size_t)kPollWord * E, sizeof(int32_t) * E, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t i = 0; i < word.size(); i++) {
      if (state) state[i] = word[i] >> kPollWordStateShift;
      if (flags) flags[i] = word[i] & ((1 << kPollWordStateShift) - 1);
    }
    return GGRS_OK;
  }
};

}  // namespace ggrs
