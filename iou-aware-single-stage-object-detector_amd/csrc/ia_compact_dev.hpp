// Device pieces of the ordered stream compaction shared by masked_conv.hip (mask -> kept pixels) and
// ssddecode.hip (row scores -> kept anchor rows): wave ballots inside a workgroup of kMaskBlock
// elements, an exclusive prefix scan over the per-workgroup counts, the ballots again for the rank.
// No atomics: the kept elements keep their order, and every run gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ia {

constexpr int kMaskBlock = 256;          // elements per workgroup of the compaction kernels

__device__ __forceinline__ int mask_popc(unsigned long long v) { return __popcll(v); }

// number of kept elements of this workgroup (one element per thread, kMaskBlock threads); the four
// popcounts are added in a fixed order.  s_wave: kMaskBlock / 64 ints of LDS.
__device__ __forceinline__ int block_keep_count(bool keep, int *s_wave)
{
    const unsigned long long bal = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mask_popc(bal);
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < kMaskBlock / 64; ++w) n += s_wave[w];
    return n;
}

// rank of this thread's element among the kept elements of its workgroup: the earlier wavefronts'
// popcounts + popcount(ballot below the lane)
__device__ __forceinline__ int block_keep_rank(bool keep, int *s_wave)
{
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = mask_popc(bal);
    __syncthreads();
    int r = 0;
    for (int w = 0; w < wave; ++w) r += s_wave[w];
    return r + mask_popc(bal & ((1ull << lane) - 1ull));
}

// one workgroup of 256 threads: block_off = exclusive prefix of block_count[0 .. nblocks), 256 at a
// time with a running carry; returns the total (in every thread).  s_v: 256 ints, s_carry: 1 int.
__device__ __forceinline__ int scan_block_counts(const int32_t *block_count, int32_t *block_off, int64_t nblocks,
                                                 int *s_v, int *s_carry)
{
    const int tid = threadIdx.x;
    if (tid == 0) *s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nblocks; base += 256) {
        const int64_t i = base + tid;
        const int v = i < nblocks ? block_count[i] : 0;
        s_v[tid] = v;
        __syncthreads();
        // Hillis-Steele inclusive scan of the 256 values
        for (int o = 1; o < 256; o <<= 1) {
            const int add = tid >= o ? s_v[tid - o] : 0;
            __syncthreads();
            s_v[tid] += add;
            __syncthreads();
        }
        const int carry = *s_carry;
        if (i < nblocks) block_off[i] = carry + s_v[tid] - v;
        __syncthreads();
        if (tid == 255) *s_carry = carry + s_v[255];
        __syncthreads();
    }
    return *s_carry;
}

}  // namespace ia
