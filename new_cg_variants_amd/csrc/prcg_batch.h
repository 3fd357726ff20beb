// What a batch of small systems (prcg_batch.cpp) borrows from the handle it was created on (prcg_engine.cpp owns the
// handle's layout): its device, its compute stream, whether it carries a communicator, and its error text.
#pragma once
#include <hip/hip_runtime_api.h>

struct prcg_handle;

namespace prcg {

struct BatchHost {
    int dev;
    hipStream_t sc;     // the handle's compute stream: every launch and copy of the batch is enqueued there
    bool comm;          // a communicator on the handle: batches are refused
};
BatchHost batch_host(const prcg_handle* h);
// sets the handle's prcg_last_error text and returns `code`
int batch_fail(prcg_handle* h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

}  // namespace prcg
