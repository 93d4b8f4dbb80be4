// cf_shared.hpp — what cf.hip (the expansion of triggers through the similarity table) and rtu2i.hip (RealTimeU2IRecall's
// trigger stage in front of it) share: the trigger limit, the keyed tables' hash and empty mark, and the
// hand-over of a batch's trigger lists in device memory.
#pragma once
#include "common.hpp"

struct pg_rtu2i;

namespace pg {

constexpr uint32_t kCfMaxTriggers = 256;
constexpr uint32_t kCfEmpty = 0xFFFFFFFFu;       // never a key: keys are local rows < rows <= UINT32_MAX

// (the multiplicative hash of exclude.hip on 32-bit rows, scaled to any slot count: rows that share their low bits, or are
// multiples of the slot count, spread over the table)
__device__ inline uint32_t cf_slot(uint32_t row, uint32_t slots) {
    return (uint32_t)(((uint64_t)(row * 0x9E3779B1u) * slots) >> 32);
}

// Trigger lists at a fixed stride with a device count per request: request q's triggers are d_rows / d_weight
// [q * stride, q * stride + min(d_count[q], stride)).  What the trigger kernel writes and the expansion kernel reads, with no
// host read-back between the two launches.
struct CfTrigDev {
    const uint32_t* d_rows = nullptr;
    const double* d_weight = nullptr;
    const uint32_t* d_count = nullptr;
    uint32_t stride = 0;
};

// rtu2i.hip.  The checks every form of the trigger stage makes, in this order, named after the entry point `who`.
int rt_check(const char* who, const pg_rtu2i* c, uint64_t rows, const void* ev_rows, const void* ev_code, const void* ev_time,
             const uint32_t* ev_off, const int64_t* now, uint32_t nq);
// The trigger kernel of nq requests over device events (indexed by the host offsets as given), enqueued on the context's
// stream: nothing synchronises.  Outputs [nq][T] / [nq]: the caller's, or with all three NULL regions of kSlotRtU2I; *out
// describes them either way.  Caller holds ctx->mu; ev_off and now must stay valid until the stream is synchronised.
int rt_triggers_enqueue_locked(const char* who, pg_ctx* ctx, pg_rtu2i* c, uint32_t rows, const uint32_t* d_ev_rows, const uint16_t* d_ev_code,
                               const double* d_ev_play_time, const int64_t* d_ev_time, const uint32_t* ev_off, const int64_t* now, uint32_t nq,
                               uint32_t* d_out_rows, double* d_out_weight, uint32_t* d_out_count, CfTrigDev* out);

}  // namespace pg
