// Host helpers shared by the launches that run several layers: the persistent ones, whose workgroups wait for each other (conv_pair.hip's
// chains, conv_run.hip), and conv_tile.hip's, which takes layer_of only.
#pragma once
#include <cstdlib>

#include "common.hpp"

namespace lav {

// LAV_CHAIN_SPIN_LIMIT, read at every launch: the bound of a wait in polls.  Test knob: 0 makes every wait that is not satisfied at
// once a time-out.
inline long long chain_spin_limit() {
    const char *lim = getenv("LAV_CHAIN_SPIN_LIMIT");
    return lim ? std::max(0ll, atoll(lim)) : (1ll << 21);
}

// the sticky {workgroups that gave up waiting, launches} words at `offset` bytes of a run's workspace; synchronises the stream
inline int read_status(const void *workspace, size_t offset, int *h_timeouts_launches2, hipStream_t st) {
    LAV_HIP(hipMemcpyAsync(h_timeouts_launches2, static_cast<const char *>(workspace) + offset, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    LAV_HIP(hipStreamSynchronize(st));
    return LAV_OK;
}

// entry i of a kernel's fixed-size per-layer arrays: the slots behind the last layer repeat it, so that the kernel may read any of them
inline int layer_of(int i, int n) { return i < n ? i : n - 1; }

}  // namespace lav
