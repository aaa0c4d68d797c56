// events_host.h -- the host side of an event-queue unit (events_device.h has the step and the kernels):
// the layout of the sessions' queue words kept between launches, and EventQueueHost, what the P2P
// engine's unit (p2p_events.hip) and the spectator engine's (spectator_events.hip) keep beside them --
// the configuration, the next call to collect, the ring, the staging area of an invocation's desync
// records, the drain's scan buffers, the staging of host-sourced calls and the state read-back.  Host
// code and plain structs only; no kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace ggrs {

constexpr int kEvMaxQueue = 100;     // MAX_EVENT_QUEUE_SIZE (p2p_session.rs:27, p2p_spectator_session.rs:21)
constexpr int kEvMinCapacity = 128;  // the ring's records per session
constexpr int kEvMaxCapacity = 1024;
// desync records a session can take from one invocation: two calls' worth of the most one call can
// compare (MAX_CHECKSUM_HISTORY_SIZE = 32 pending reports)
constexpr int kEvStageD = 64;
constexpr int kEvScanBlock = 256;    // sessions per block of the drain's scan

// the sessions' words kept between launches, [fields][S] rows
enum EvField : int {
  kEvHead = 0,     // the ring slot of the oldest record
  kEvLen,          // records queued
  kEvDropped,      // records a full ring dropped
  kEvStatus,       // 0, GGRS_EVENTS_LOST
  kEvClosedCall,   // the call at which the endpoint towards the remote players (the host) closed (-1: open)
  kEvFields
};
// the staging area's planes, [kEvStagePlanes][kEvStageD][S]
enum EvStagePlane : int { kEvStageCall = 0, kEvStageFrame, kEvStageChecksums, kEvStagePlanes };

struct EventQueueHost {
  int32_t on = 0;
  int32_t capacity = 0;
  int32_t next = 0;              // the next call to collect
  int64_t list_from = 0;         // the engine's own desync list: every record below this index was collected
  size_t S = 0;
  ggrs_event_record_t* ring = nullptr;  // [capacity][S]
  int32_t* st = nullptr;         // [kEvFields][S]
  int32_t* stage = nullptr;      // [kEvStagePlanes][kEvStageD][S], allocated by the first invocation with records
  int32_t* stage_count = nullptr;  // [S] records bucketed for the session by this invocation (0 between them)
  int64_t* block_offs = nullptr;   // [grid_of(S, kEvScanBlock)] the drain's block sums, then their exclusive scan
  unsigned long long* meta = nullptr;  // [2] the drain: records queued, records taken
  uint8_t* staging = nullptr;    // host-sourced rows and drained records
  size_t staging_bytes = 0;

  void release() {
    void* bufs[] = {ring, st, stage, stage_count, block_offs, meta, staging};
    for (void* b : bufs)
      if (b) (void)hipFree(b);
    ring = nullptr;
    st = stage = stage_count = nullptr;
    block_offs = nullptr;
    meta = nullptr;
    staging = nullptr;
    staging_bytes = 0;
    on = 0;
    S = 0;
  }
  // Every queue empty, nothing dropped or lost, the endpoint open.
  int configure(size_t sessions, int32_t cap, hipStream_t stream) {
    if (cap < kEvMinCapacity || cap > kEvMaxCapacity)
      return set_error(GGRS_E_INVALID, "the event queue's capacity must be in %d..%d, got %d", kEvMinCapacity, kEvMaxCapacity,
                       cap);
    if (S != sessions || capacity != cap) release();
    // (each buffer on its own: one that failed to allocate is the only one a later call allocates)
    if (!ring) HIP_TRY(hipMalloc(&ring, sizeof(ggrs_event_record_t) * (size_t)cap * sessions));
    if (!st) HIP_TRY(hipMalloc(&st, sizeof(int32_t) * (size_t)kEvFields * sessions));
    if (!stage_count) HIP_TRY(hipMalloc(&stage_count, sizeof(int32_t) * sessions));
    if (!block_offs) HIP_TRY(hipMalloc(&block_offs, sizeof(int64_t) * (size_t)grid_of((int64_t)sessions, kEvScanBlock)));
    if (!meta) HIP_TRY(hipMalloc(&meta, sizeof(unsigned long long) * 2));
    S = sessions;
    capacity = cap;
    std::vector<int32_t> w0((size_t)kEvFields * sessions, 0);
    for (size_t i = 0; i < sessions; i++) w0[(size_t)kEvClosedCall * sessions + i] = -1;
    HIP_TRY(hipMemcpyAsync(st, w0.data(), sizeof(int32_t) * w0.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(ring, 0, sizeof(ggrs_event_record_t) * (size_t)cap * sessions, stream));
    HIP_TRY(hipMemsetAsync(stage_count, 0, sizeof(int32_t) * sessions, stream));
    HIP_TRY(hipMemsetAsync(meta, 0, sizeof(unsigned long long) * 2, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    on = 1;
    next = 0;
    list_from = 0;
    return GGRS_OK;
  }
  // Calls first_call .. first_call + n - 1: in order, each once.
  int check_calls(int32_t first_call, int32_t n) const {
    if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
    if (first_call != next)
      return set_error(GGRS_E_INVALID, "events are collected in call order, each call once (expected call %d, got %d)", next,
                       first_call);
    return GGRS_OK;
  }
  int need_stage() {
    if (!stage) HIP_TRY(hipMalloc(&stage, sizeof(int32_t) * (size_t)kEvStagePlanes * kEvStageD * S));
    return GGRS_OK;
  }
  // The sessions' words [S] each and the queues [capacity][S] in queue order (zero past a queue's
  // length); any pointer may be null
  int read(int32_t* length, int32_t* dropped, int32_t* status, int32_t* closed_call, ggrs_event_record_t* queue,
           hipStream_t stream) const {
    int32_t* const dst[kEvFields] = {nullptr, length, dropped, status, closed_call};
    for (int f = 0; f < kEvFields; f++)
      if (dst[f]) HIP_TRY(hipMemcpyAsync(dst[f], st + (size_t)f * S, sizeof(int32_t) * S, hipMemcpyDeviceToHost, stream));
    std::vector<int32_t> hl;
    std::vector<ggrs_event_record_t> raw;
    hipError_t rc = hipSuccess;
    if (queue) {
      static_assert(kEvLen == kEvHead + 1, "head and length are read in one copy");
      hl.resize(2 * S);
      raw.resize((size_t)capacity * S);
      rc = hipMemcpyAsync(hl.data(), st + (size_t)kEvHead * S, sizeof(int32_t) * 2 * S, hipMemcpyDeviceToHost, stream);
      if (rc == hipSuccess)
        rc = hipMemcpyAsync(raw.data(), ring, sizeof(ggrs_event_record_t) * raw.size(), hipMemcpyDeviceToHost, stream);
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (before the vectors can be freed)
    HIP_TRY(rc);
    HIP_TRY(waited);
    if (queue)
      for (size_t s = 0; s < S; s++) {
        const int32_t head = hl[s], len = hl[S + s];
        for (int32_t i = 0; i < capacity; i++)
          queue[(size_t)i * S + s] = i < len ? raw[(size_t)((head + i) % capacity) * S + s] : ggrs_event_record_t{};
      }
    return GGRS_OK;
  }
};

}  // namespace ggrs
