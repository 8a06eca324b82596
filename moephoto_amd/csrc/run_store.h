// run_store.h -- the run of elements a thread writes at once (the stitch fold's edges, the luma-only steps' split and merge, the polyphase kernels): whole 16-byte stores
// where the address allows them, and the one store of a row's ragged end.
#pragma once
#include "common.h"

// A run of N elements a thread writes at once: aligned vector stores where the address allows it, element by element elsewhere (a canvas whose width is not a
// multiple of 8, a base in the middle of a buffer).  The vector path stores words, not the struct: a struct copy is taken apart into element stores, the ones that
// equal the fallback's are then sunk behind the branch, and the "vector" path keeps 16-byte stores for part of the run only (samples of the 8K canvas: 257 us for 211).
// (a run of four bytes -- four u8 chroma samples -- is one word)
template <typename T, int N> struct alignas((sizeof(T) * N) % 16 == 0 ? 16 : (sizeof(T) * N) % 8 == 0 ? 8 : 4) StitchRun { T e[N]; };

template <typename T, int N>
__device__ __forceinline__ void stitch_store(T* p, const StitchRun<T, N>& v)
{
    constexpr int A = alignof(StitchRun<T, N>), NV = sizeof(StitchRun<T, N>) / A;
    typedef unsigned vec_t __attribute__((ext_vector_type(A / 4)));
    if (((uintptr_t)p & (A - 1)) == 0) {
        vec_t q[NV];
        __builtin_memcpy(q, &v, sizeof(v));
#pragma unroll
        for (int k = 0; k < NV; ++k) ((vec_t*)p)[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = v.e[k];
    }
}

// The first n pixels of a run of eight, N / 8 elements each: whole runs through stitch_store, the ragged end element by element (constant indices in loops of eight
// that unroll: a run indexed by a loop variable is moved to LDS)
template <typename T, int N>
__device__ __forceinline__ void stitch_store_n(T* p, const StitchRun<T, N>& v, int n)
{
    constexpr int G = N / 8;
    if (n == 8) stitch_store(p, v);
    else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e >= n) break;
#pragma unroll
            for (int c = 0; c < G; ++c) p[e * G + c] = v.e[e * G + c];
        }
    }
}
