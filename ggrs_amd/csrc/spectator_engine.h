// spectator_engine.h -- the spectator engine object shared by spectator.hip (the sessions' kernel
// and the table-fed inputs) and spectator_ingest.hip (the packet feed).  Host-side only; no kernels
// here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "events_host.h"
#include "poll_host.h"

struct ggrs_spectator_engine {
  ggrs_spectator_config_t cfg{};
  int F = 1, cap = 256, acap = 256;
  hipStream_t stream = nullptr;
  uint32_t* cur = nullptr;
  int32_t* sst = nullptr;
  uint32_t* rows = nullptr;
  int4* recv = nullptr;   // [acap / 4][S]
  int4* notes = nullptr;
  uint8_t* adv = nullptr;
  uint16_t* ck = nullptr;
  uint8_t* staging = nullptr;
  size_t staging_bytes = 0;
  int32_t calls = 0;
  int32_t next_input_frame = 0;
  int32_t next_arrival_call = 0;
  ggrs::SpanTimer timer;
  // the packet feed (ggrs_spectator_set_packet_feed, spectator_ingest.hip)
  int32_t pkt = 0;                 // the sessions' inputs and arrivals come from packets
  int32_t pkt_maxp = 0;            // the hosts' max_prediction
  ggrs::PacketFeedState feed;      // (last: the session's input window ends here; stop: the call whose packet
                                   // stopped the session; staged beside the packets: the calls' notes)
  // the endpoint poll (ggrs_spectator_set_endpoint_poll, spectator_poll.hip): one endpoint per session
  ggrs::PollHost poll;
  // the event queue (ggrs_spectator_set_event_queue, spectator_events.hip): every session's GgrsEvent queue
  ggrs::EventQueueHost evq;
};

namespace ggrs {

// The recv_upto word of a call at which the feed stopped its session (and of the calls after it): no
// frame number, so the kFeed form of spectator_kernel tells it from an arrival.
constexpr int32_t kSpecFeedStop = INT32_MIN;

int spectator_ingest_free(ggrs_spectator_engine* e);
// spectator_poll.hip: free the endpoint poll's buffers
int spectator_poll_free(ggrs_spectator_engine* e);
// spectator_events.hip: free the event queue's buffers
int spectator_events_free(ggrs_spectator_engine* e);

}  // namespace ggrs
