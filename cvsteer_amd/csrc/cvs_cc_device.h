// cvs_cc_device.h -- __device__ helpers of the union-find labelling, shared by the kernels of cvs_kernels_components.hip and
// cvs_kernels_link.hip: finds and unions on a tile in LDS and on the parent plane in memory, the read-only root walk, the order-keeping
// bits of a float, and the runs of equal keys inside a wave.  Device code only; included behind <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

namespace cvs {

// ---- a tile in LDS: workgroup-scope atomics on tile-local indices ----
__device__ __forceinline__ int lds_get(int* L, int i) { return __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(int* L, int i)
{
    for (;;) {
        const int p = lds_get(L, i);
        if (p == i) return i;
        i = p;
    }
}

__device__ __forceinline__ void lds_union(int* L, int a, int b)
{
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;   // a was still a root: linked
        a = old;                // somebody else linked a first: go on from there
    }
}

// ---- the parent plane while other workgroups of the same launch change it: agent-scope atomics only ----
__device__ __forceinline__ int g_get(int32_t* P, int i) { return __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(int32_t* P, int i)
{
    for (;;) {
        const int p = g_get(P, i);
        if (p == i) return i;
        i = p;
    }
}

__device__ __forceinline__ void g_union(int32_t* P, int a, int b)
{
    for (;;) {
        a = g_find(P, a);
        b = g_find(P, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// ---- the parent plane once it is final: read-only, plain loads behind the launch boundary ----
__device__ __forceinline__ int root_of(const int32_t* P, int i)
{
    int p = P[i];
    while (p != i) {
        i = p;
        p = P[i];
    }
    return i;
}

// ---- statistics: floats as ordered integers, runs of equal keys in a wave ----
__device__ __forceinline__ unsigned ordered_bits(float f)   // monotone in f for every non-NaN f, -0.0f below +0.0f; never 0
{
    const unsigned u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ordered_value(unsigned o) { return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o); }

// the lane's run among the wave's 64 keys: head = first lane of it, end = one past its last lane
__device__ __forceinline__ void run_of(int key, int lane, bool& head, int& end)
{
    const int prev = __shfl_up(key, 1, 64);
    head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    end = above ? __ffsll((long long)above) - 1 : 64;
}

}  // namespace cvs
