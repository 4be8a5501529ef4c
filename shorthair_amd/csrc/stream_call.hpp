// The guard of one call that enqueues work on a caller's stream: what csrc/packet_host.cpp needs of the
// library's Context, which stays private to csrc/cauchy_256_host.cpp (where this type is implemented).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

namespace sh {

// Construct one after the arguments are checked, and return rc if it is not 0 (-2: no usable GPU; it has
// been reported on stderr). For its lifetime
//   - the library's device is the calling thread's current device (the thread's own comes back after it);
//   - `stream`'s state exists, and `errors` is that stream's device counter of malformed items;
//   - the stream's mutex is held. A call enqueues the kernels that add to `errors` under it, and
//     cauchy_256_batch_errors enqueues its read-and-clear under it: the counts of a call land either all
//     before a read or all after its clear, never astride, whichever threads make the calls.
// counts = false is for a call that adds nothing to `errors`: it gets the device and the stream only, and
// takes no lock (`errors` stays null).
class StreamCall {
public:
    explicit StreamCall(void *stream, bool counts = true);
    ~StreamCall();
    StreamCall(const StreamCall &) = delete;
    StreamCall &operator=(const StreamCall &) = delete;

    int rc = 0;
    hipStream_t stream = nullptr;
    int *errors = nullptr;

private:
    struct Held;  // the device scope and the lock
    std::unique_ptr<Held> held_;
};

}  // namespace sh
