// Order-preserving compaction, shared by occupancy_kernels.hip (the kept points of a pass), grid_resample_kernels.hip (mask ->
// links) and grid_components_kernels.hip (the roots' ranks): count the set flags per workgroup, scan the counts in one
// workgroup, give every set flag its rank. Three stream-ordered launches; nothing waits for another workgroup and nothing
// appends with atomics, so the ranks are those of the items' own order and two runs give the same bits.
//
// Workgroup b of the count and of the rank launch (256 threads) owns items [b * 1024, (b + 1) * 1024) in four rounds of 256:
// wavefront w of round r holds 64 consecutive items, whose flags are the 64-bit ballot number r * 4 + w of the workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nerf {
namespace {

constexpr int kCompactItems = 1024;      // items per workgroup: 4 rounds of 256 threads

inline int64_t compact_blocks(int64_t n) { return (n + kCompactItems - 1) / kCompactItems; }      // workgroups = entries of the counts

// the item of the calling thread in round r
__device__ __forceinline__ int64_t compact_item(int r) { return (int64_t)blockIdx.x * kCompactItems + r * 256 + threadIdx.x; }

// ---- count: every wavefront passes the set flags it counted in its four ballots; thread 0 stores the workgroup's count ----
__device__ __forceinline__ void compact_store_count(int wave_sum, int* block_counts) {
    __shared__ int wave_count[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = wave_sum;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

// ---- scan: one workgroup of 1024 threads turns counts[0..n) into exclusive offsets, in place ----
// Thread t owns the `per` consecutive counts from t * per (none once those are past n). Returns the calling thread's inclusive
// partial sum: in thread 1023 that is the total.
__device__ __forceinline__ int compact_scan(int* counts, int64_t n) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += counts[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {      // inclusive scan of the 1024 partial sums
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int c = counts[i];
        counts[i] = run;
        run += c;
    }
    return part[t];
}

// ---- ranks: the workgroup's 16 ballots and the rank of the first flag of each, in LDS ----
struct CompactRanks {
    const unsigned long long* words;
    const int* word_off;
    // is the flag of the calling lane's item of round r set, and its rank among all set flags
    __device__ __forceinline__ bool kept(int r) const { return (words[r * 4 + (threadIdx.x >> 6)] >> (threadIdx.x & 63)) & 1ull; }
    __device__ __forceinline__ int rank(int r) const {
        const int q = r * 4 + (threadIdx.x >> 6);
        return word_off[q] + __popcll(words[q] & ((1ull << (threadIdx.x & 63)) - 1ull));
    }
};

// thread 0 turns the 16 ballots (LDS, written before the call) into their 16 offsets, from this workgroup's scanned count
__device__ __forceinline__ CompactRanks compact_word_offsets(const unsigned long long* words, const int* block_offsets) {
    __shared__ int word_off[16];
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = block_offsets[blockIdx.x];
        for (int q = 0; q < 16; ++q) {
            word_off[q] = run;
            run += __popcll(words[q]);
        }
    }
    __syncthreads();
    return CompactRanks{words, word_off};
}

// from the calling thread's flags of the four rounds
__device__ __forceinline__ CompactRanks compact_ranks(const bool (&flag)[4], const int* block_offsets) {
    __shared__ unsigned long long words[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned long long ballot = __ballot(flag[r]);
        if ((threadIdx.x & 63) == 0) words[r * 4 + (threadIdx.x >> 6)] = ballot;
    }
    return compact_word_offsets(words, block_offsets);
}

// from the workgroup's 16 ballots as a count launch left them in memory
__device__ __forceinline__ CompactRanks compact_ranks(const unsigned long long* block_words, const int* block_offsets) {
    __shared__ unsigned long long words[16];
    if (threadIdx.x < 16) words[threadIdx.x] = block_words[threadIdx.x];
    return compact_word_offsets(words, block_offsets);
}

}  // namespace
}  // namespace nerf
