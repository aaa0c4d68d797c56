// poll_device.h -- one endpoint's poll step, shared by the units that run UdpProtocol's timers on the
// device (p2p_poll.hip; the spectator endpoints can take it as they take ingest_device.h and
// emit_device.h): UdpProtocol::poll (src/network/protocol.rs:329-376), the clock bookkeeping of
// handle_message (:534-551), on_input's running_last_input_recv and send_input_ack (:608, :634) and
// disconnect (:311-319), over one clock per poll.  All times are u64 milliseconds; every comparison is
// strict, as the reference's are.
//
// send_keep_alive (:344-347) is not here because it cannot fire: last_send_time is set by every
// queue_message, send_quality_report sets running_last_quality_report and then queues, and the
// constructor initialises the two in that order, so last_send_time >= running_last_quality_report at
// every check; both intervals are 200 ms, so either the report fired in this poll (last_send_time is
// then later than poll's `now`) or last_send_time + 200 >= running_last_quality_report + 200 >= now
// (DESIGN.md section 3 "Endpoint poll"; tests/test_endpoint_poll_model.py pins it on a literal model).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ggrs_amd.h"

namespace ggrs {

constexpr uint64_t kPollRetryMs = 200;      // RUNNING_RETRY_INTERVAL (protocol.rs:17)
constexpr uint64_t kPollReportMs = 200;     // QUALITY_REPORT_INTERVAL (:19)
constexpr uint64_t kPollShutdownMs = 5000;  // UDP_SHUTDOWN_TIMER (:21)
// the endpoint's flag word: disconnect_notify_sent, disconnect_event_sent, then ProtocolState
constexpr uint32_t kPollNotifySent = 1, kPollEventSent = 2;
constexpr int kPollStateShift = 2;
// what a step returns beside the GGRS_NET_* bits (bits 0-3)
constexpr uint32_t kPollResend = 16, kPollSendAck = 32, kPollSendReport = 64;

struct PollEndpoint {
  uint64_t last_recv;        // last_recv_time
  uint64_t last_input_recv;  // running_last_input_recv
  uint64_t last_report;      // running_last_quality_report
  uint64_t shutdown;         // shutdown_timeout
  uint32_t word;             // kPollNotifySent | kPollEventSent | state << kPollStateShift
  int32_t closed_call;       // the call at which the endpoint went Running -> Disconnected (-1)
};

// Call c's poll of one endpoint at clock `now`: any = a message was accepted, decoded = an Input
// among them was decoded, ext = a remote player's Event::Disconnected bit is in the call's events byte
// already.  Returns GGRS_NET_* | kPollResend | kPollSendAck | kPollSendReport; GGRS_NET_DISCONNECTED
// says the caller has to add the remote players' bits to the events byte.
__device__ __forceinline__ uint32_t poll_endpoint_step(PollEndpoint& ep, uint64_t now, uint64_t timeout, uint64_t notify,
                                                       int32_t c, bool any, bool decoded, bool ext) {
  const uint32_t state = ep.word >> kPollStateShift;
  if (state == GGRS_ENDPOINT_SHUTDOWN) return 0;  // 0. (:538-541, :373)
  uint32_t out = 0;
  if (any) {  // 1. handle_message (:544-551)
    ep.last_recv = now;
    if ((ep.word & kPollNotifySent) && state == GGRS_ENDPOINT_RUNNING) {
      ep.word &= ~kPollNotifySent;
      out |= GGRS_NET_RESUMED;
    }
  }
  if (decoded) {  // 2. on_input (:608, :634)
    ep.last_input_recv = now;
    out |= kPollSendAck;
  }
  if (state == GGRS_ENDPOINT_RUNNING) {  // 4. poll (:332-367)
    if (ep.last_input_recv + kPollRetryMs < now) {
      out |= kPollResend;
      ep.last_input_recv = now;
    }
    if (ep.last_report + kPollReportMs < now) {
      out |= kPollSendReport;
      ep.last_report = now;
    }
    if (!(ep.word & kPollNotifySent) && ep.last_recv + notify < now) {
      out |= GGRS_NET_INTERRUPTED;
      ep.word |= kPollNotifySent;
    }
    if (ext) ep.word |= kPollEventSent;  // (on_input's disconnect_requested, :569-574)
    if (!(ep.word & kPollEventSent) && ep.last_recv + timeout < now) {
      out |= GGRS_NET_DISCONNECTED;
      ep.word |= kPollEventSent;
      ext = true;
    }
    if (ext) {  // the session handles the event: disconnect (:311-319)
      ep.word = (ep.word & ((1u << kPollStateShift) - 1u)) | (uint32_t)GGRS_ENDPOINT_DISCONNECTED << kPollStateShift;
      ep.shutdown = now + kPollShutdownMs;
      ep.closed_call = c;
    }
  } else if (ep.shutdown < now) {  // 5. Disconnected at entry (:368-372)
    ep.word = (ep.word & ((1u << kPollStateShift) - 1u)) | (uint32_t)GGRS_ENDPOINT_SHUTDOWN << kPollStateShift;
    out |= GGRS_NET_SHUTDOWN;
  }
  return out;
}

}  // namespace ggrs
