// Host-only planning of a chunked walk's scratch, free of the HIP runtime so that tests/sanitize/scratch_plan_harness.cpp compiles it
// alone: how many items of a batch one chunk takes, and where each region of the arena starts.
#pragma once
#include <stddef.h>
#include <algorithm>
namespace alch {
// Items per chunk at per_item_bytes of scratch each within budget_bytes: at most the batch, at least one (a larger item runs alone).
inline size_t scratch_chunk(size_t budget_bytes, size_t batch, size_t per_item_bytes) {
    return std::min(batch, std::max<size_t>(1, budget_bytes / per_item_bytes));
}
// Ciphertexts per launch pair of the fused paths, whose kernels use 32-bit byte offsets per array and groups of 8: a multiple of 8.
inline size_t fused_chunk(size_t ring_chunk, size_t pair_bytes, size_t batch) {
    const size_t cap = std::max<size_t>(8, (((size_t)1 << 32) - 1) / pair_bytes / 8 * 8);
    return std::min(std::min(ring_chunk, cap), (batch + 7) / 8 * 8);
}
// The regions of an arena of `chunk` items, in layout order (0 bytes: a region this call does not need).  A walk reserves chunk * per_ct
// bytes, takes its regions and stops on the host unless matches(per_ct): the sum and the carve are one fact.
struct Carve {
    char* at;
    size_t chunk, sum = 0;
    Carve(void* base, size_t chunk_) : at(static_cast<char*>(base)), chunk(chunk_) {}
    char* take(size_t bytes_per_item) { char* p = at; at += chunk * bytes_per_item; sum += bytes_per_item; return p; }
    size_t taken_per_item() const { return sum; }
    bool matches(size_t per_item) const { return sum == per_item; }
};
}  // namespace alch
