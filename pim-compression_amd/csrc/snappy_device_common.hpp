// snappy_device_common.hpp -- the device building blocks every kernel header shares: memory primitives, the work counter
// draw, the fence between a wavefront's stores and its own loads, scans, the prefix search, varints and the two copies.
// __device__ __forceinline__ pieces only (no kernel lives here); snappy_kernels.hpp, snappy_ranges.hpp, snappy_update.hpp
// and snappy_raw.hpp include it directly.  tests/test_device_common_emulated.py holds each piece to a numpy model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snappy_hip {

constexpr uint32_t kWave = 64;

// ---------------------------------------------------------------------------
// memory primitives
// ---------------------------------------------------------------------------

// broadcast lane 0's value; marks the value wave-uniform for the compiler (SGPR)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// unaligned little-endian loads (gfx950 runs with unaligned VMEM/DS access enabled)
__device__ __forceinline__ uint32_t ld32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t* p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// wave-uniform load of 4 bytes at a uniform address
__device__ __forceinline__ uint32_t uld32(const uint8_t* p) { return uni(ld32(p)); }
__device__ __forceinline__ uint64_t uld64(const uint8_t* p)
{
    const uint64_t v = ld64(p);
    return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32);
}

// unaligned 16-byte load and store (one global_load_dwordx4 / global_store_dwordx4)
__device__ __forceinline__ uint4 ld128(const uint8_t* p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void st128(uint8_t* p, uint4 v) { __builtin_memcpy(p, &v, 16); }

// A pointer the kernel reads from a descriptor in memory, not from its arguments, is generic to the compiler, and generic
// accesses become flat_* instructions -- which K2's decoder must not use (it relies on global_* operations of a wavefront
// completing in order, tests/test_abi_symbols.py).  Loaded as a pointer to global memory, it keeps that knowledge.
template <class T>
__device__ __forceinline__ T* load_global_ptr(T* const* field)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(1))) T* global_t;
    return (T*)*reinterpret_cast<const global_t*>(reinterpret_cast<uintptr_t>(field));
#else
    return *field;
#endif
}

// the parts of a call's scratch start at multiples of 256 bytes
__host__ __device__ inline uint64_t round256(uint64_t v) { return (v + 255u) & ~255ull; }

// ---------------------------------------------------------------------------
// persistent wavefronts
// ---------------------------------------------------------------------------

// the next work item of a persistent wavefront: lane 0 draws from the launch's counter, every lane gets the number (SGPR)
__device__ __forceinline__ uint32_t draw_work(uint32_t* counter, uint32_t lane)
{
    uint32_t drawn = 0;
    if (lane == 0) drawn = atomicAdd(counter, 1u);
    return uni(drawn);
}

// what this wavefront has stored is in memory before any of its lanes loads it again through another lane's address
__device__ __forceinline__ void stores_landed()
{
#ifndef SNAPPY_EMU
    __builtin_amdgcn_s_waitcnt(0);
#endif
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------
// scans and the search over their results
// ---------------------------------------------------------------------------

// inclusive scan of one u32 per lane over the wavefront (every lane active)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane)
{
#ifdef SNAPPY_EMU
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, (int)d);
        if (lane >= d) v += t;
    }
#else
    (void)lane;
    // Hillis-Steele inside each row of 16 lanes (row_shr:1,2,4,8; lanes without a source keep the 0 of `old`), then the row
    // totals travel up: lane 15 of rows 0 and 2 into rows 1 and 3, lane 31 into rows 2 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
#endif
    return v;
}

// Exclusive scan of one u64 per thread over the 1024 threads of the workgroup; `total` = the workgroup's sum, in every
// thread.  wave_sums: 16 shared words.  Two barriers; a planner that loops over more than 1024 elements keeps its carry in
// a register (carry += total) and may call again at once: the first barrier guards wave_sums against the trip before.
__device__ __forceinline__ uint64_t workgroup_exclusive_scan(uint64_t mine, uint64_t* wave_sums, uint64_t& total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = mine;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, (int)d);
        const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), (int)d);
        if (lane >= d) x += ((uint64_t)hi << 32) | lo;
    }
    __syncthreads();
    if (lane == 63) wave_sums[wave] = x;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (uint32_t w = 0; w < 16; ++w) {
        if (w < wave) before += wave_sums[w];
        total += wave_sums[w];
    }
    return before + x - mine;
}

// the owner of work item p in an exclusive prefix of work counts: the last i < count with prefix[i] <= p (owners of no work
// share their prefix with the next one).  p is wave-uniform.  kVectorLoads: each step reads through uld64 (a vector load and a
// readfirstlane), as decompress_ranges_kernel always did; otherwise plainly, which the compiler turns into scalar loads, as
// the raw kernels always did.  Each caller keeps the instructions it was measured with: one form for all is a change of speed
// (the raw fragment kernel on vector loads: 1 % slower on a compress batch) and wants a measurement of its own.
template <bool kVectorLoads>
__device__ __forceinline__ uint32_t prefix_owner(const uint64_t* __restrict__ prefix, uint32_t count, uint32_t p)
{
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t first = kVectorLoads ? uld64(reinterpret_cast<const uint8_t*>(prefix + mid)) : prefix[mid];
        if (first <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// varints (the stream headers; the host's are in dropin_plan.hpp)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t varint32_len(uint32_t v)
{
    uint32_t n = 1;
    while (v >= 0x80u) { v >>= 7; ++n; }
    return n;
}
__device__ __forceinline__ uint32_t put_varint32(uint8_t* dst, uint32_t v)
{
    uint32_t k = 0;
    while (v >= 0x80u) { dst[k++] = (uint8_t)(v | 0x80u); v >>= 7; }
    dst[k++] = (uint8_t)v;
    return k;
}

// ---------------------------------------------------------------------------
// copies, both ends at any alignment
// ---------------------------------------------------------------------------

// len bytes by a workgroup of 256 threads: bytes up to the destination's first 16-byte boundary, 16-byte stores on the
// aligned middle, bytes behind it
__device__ __forceinline__ void workgroup_copy(uint8_t* dst, const uint8_t* src, uint32_t len)
{
    const uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);   // bytes until dst is 16-byte aligned
    const uint32_t h = head < len ? head : len;
    if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t body = (len - h) & ~15u;
    for (uint32_t i = threadIdx.x * 16; i < body; i += 256 * 16)
        *reinterpret_cast<uint4*>(dst + h + i) = ld128(src + h + i);
    const uint32_t done = h + body;
    if (done + threadIdx.x < len) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

// n bytes by the whole wavefront: 16 bytes per lane and step, the last step clamped back to end at n (it rewrites bytes
// with the same values)
__device__ __forceinline__ void wave_copy(uint8_t* t, const uint8_t* s, uint32_t n, uint32_t lane)
{
    if (n >= 16u) {
        for (uint32_t i = 16u * lane; i < n; i += 16u * kWave) {
            const uint32_t o = i < n - 16u ? i : n - 16u;
            st128(t + o, ld128(s + o));
        }
    } else if (lane < n) {
        t[lane] = s[lane];
    }
}

}  // namespace snappy_hip
