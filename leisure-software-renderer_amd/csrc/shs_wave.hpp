// shs_wave.hpp -- wavefront (64-lane) helpers shared by the legacy and library raster kernels:
// in-wave LDS hand-off, the wave and block prefix sums, the pair-run bitmap, ballot-based appends and the
// order-preserving 64-bit depth key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shs_dev {

// LDS hand-off between lanes of ONE wave: the wave's LDS operations execute in order, so only the
// compiler must be kept from reordering (no s_barrier: waves of a block may diverge).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_wave_barrier();
    __asm__ volatile("" ::: "memory");
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull));
}

// Inclusive prefix sum over the wave's 64 lanes (converged wave): lane l gets v[0] + ... + v[l].
// (lane: the caller's, where it has one -- recomputed here it costs the raster kernels code and registers.)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += up;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) { return wave_incl_sum(v, __lane_id()); }

// A 256-thread block's four per-wave slots, slot[STRIDE * w] for wave w (complete: a barrier since they
// were written): the sum of the slots before the calling wave's; the block's total in tot.
template <int STRIDE>
__device__ __forceinline__ uint32_t wave_slots_before(const uint32_t *slot, int wave, uint32_t &tot) {
    uint32_t before = 0u;
    tot = 0u;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        const uint32_t p2 = slot[STRIDE * w2];
        if (w2 < wave) before += p2;
        tot += p2;
    }
    return before;
}

// Block exclusive prefix of the 256 threads' v through four per-wave slots (one barrier; the slots are free
// on entry, and again after the next barrier); the block's total in tot.
template <int STRIDE>
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t *slot, uint32_t v, int lane, int wave, uint32_t &tot) {
    const uint32_t incl = wave_incl_sum(v, lane);
    if (lane == 63) slot[STRIDE * wave] = incl;
    __syncthreads();
    return wave_slots_before<STRIDE>(slot, wave, tot) + incl - v;
}

// Pair runs.  The (candidate, pixel) pairs of a pass are numbered end to end, and a run of len pairs from
// pair `start` belongs to `owner` (a row segment or a staged box): mark_run sets its start bit in the
// bitmap over the pairs and names it the owner of every bitmap word whose first pair is in the run;
// pair_owner finds the owner of lane `lane`'s pair in the 64-pair window from pair k0 -- the window's
// word's first owner + the starts in the word up to the pair.  Own: the owner word (the caller's LDS budget).
template <class Own>
__device__ __forceinline__ void mark_run(unsigned long long *bits, Own *wown, uint32_t start, uint32_t len, uint32_t owner) {
    atomicOr(&bits[start >> 6], 1ull << (start & 63u));
    for (uint32_t wd = (start + 63u) >> 6; wd * 64u < start + len; ++wd) wown[wd] = (Own)owner;
}
template <class Own>
__device__ __forceinline__ int pair_owner(const unsigned long long *bits, const Own *wown, int k0, int lane) {
    const unsigned long long wb = bits[k0 >> 6];
    const unsigned long long upto = ((2ull << lane) - 1ull) & ~1ull;   // bits 1..lane
    return (int)wown[k0 >> 6] + __popcll(wb & upto);
}

// Wave-aggregated appends to NK per-key counters (call with the whole wave converged).  Lanes with
// key[k] >= 0 get a unique slot of counter[key[k]]; each distinct key costs ONE returning atomic, and
// all of them are issued before any return value is consumed (one memory round trip in total).
template <int NK>
__device__ __forceinline__ void wave_append(uint32_t *counter, const int (&key)[NK], uint32_t (&slot)[NK]) {
    const int lane = __lane_id();
    uint32_t add[NK], rank[NK], leader[NK], ret[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        add[k] = 0u; rank[k] = 0u; leader[k] = 0u;
        uint64_t pending = __ballot(key[k] >= 0);
        while (pending) {
            const int first = __ffsll((unsigned long long)pending) - 1;
            const int lk = __shfl(key[k], first);
            const uint64_t peers = __ballot(key[k] == lk) & pending;
            if (lane == first) add[k] = (uint32_t)__popcll(peers);
            if ((peers >> lane) & 1ull) { leader[k] = (uint32_t)first; rank[k] = lanes_below(peers); }
            pending &= ~peers;
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) ret[k] = add[k] ? atomicAdd(&counter[key[k]], add[k]) : 0u;
#pragma unroll
    for (int k = 0; k < NK; ++k) slot[k] = __shfl(ret[k], (int)leader[k]) + rank[k];
}

// Single-counter wave append (converged wave): slot for lanes with want.
__device__ __forceinline__ uint32_t wave_append1(uint32_t *counter, bool want) {
    const uint64_t m = __ballot(want);
    if (!m) return 0u;
    const int first = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0u;
    if (__lane_id() == first) base = atomicAdd(counter, (uint32_t)__popcll(m));
    return __shfl(base, first) + lanes_below(m);
}

// Order-preserving key of a strict-less z test run in submission order: the test keeps, per pixel,
// the lexicographic minimum of (z, submission index) (the first fragment with the minimal z wins), so
// a 64-bit key (orderable z bits << 32 | index) resolved by atomic min is exact and independent of
// the order candidates are processed in.  -0 and +0 compare equal in the reference, so -0 maps to
// +0's key.
constexpr unsigned long long KEY_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long z_key(float z, uint32_t id) {
    uint32_t b = __float_as_uint(z);
    b = (b << 1) == 0u ? 0u : b;                                 // -0 -> +0
    const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)ord << 32) | id;
}

}  // namespace shs_dev
