// kernels/stream.hpp — what the hops of the streaming solve sweeps of all three generations share (kernels/narrow.hpp, narrow2.hpp,
// narrow3.hpp): the rotation of the software pipeline's register arrays.
// (The pack prologue, the staging rounds and the hop loops are still written out in each of the six bodies: moved into forceinline
// pieces they compile to other instruction streams, the hop loops alone already — NOTES.md round 7, profiles/r07_stream_scaffold.txt.)
// Part of kernels.hpp (include that, not this file: the parts build on each other in its order).
#pragma once

namespace bddmma {

// Rotation of a pipeline register array by one hop, at the end of the hop: a[i] <- a[i + 1].  The last element takes `newest` (an offset
// read from the hop window), or keeps its value until the next hop's prefetch overwrites it.  Elements may themselves be arrays (one
// register set per lane group of the hop).  Inside a trip of the unrolled hop loop the rotation is renamed away.
template <typename T>
__device__ __forceinline__ void shift_put(T& dst, const T& src) { dst = src; }
template <typename T, int R>
__device__ __forceinline__ void shift_put(T (&dst)[R], const T (&src)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r) dst[r] = src[r];
}
template <typename T, int N>
__device__ __forceinline__ void shift(T (&a)[N])
{
#pragma unroll
    for (int i = 0; i + 1 < N; ++i) shift_put(a[i], a[i + 1]);
}
template <typename T, int N>
__device__ __forceinline__ void shift(T (&a)[N], T newest)
{
    shift(a);
    a[N - 1] = newest;
}

}  // namespace bddmma
