// The action-prefetch ring of the fused rollout kernels (lz_kernels.hip: rollout_loop,
// split_loop): the LDS-DMA primitives, the explicit vmcnt waits, and ActRing -- the one
// definition of the ring's constants, prologue fill, per-step wait, refill and source
// arithmetic that both loops use.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lz_body.h"

namespace lz {

typedef float f2v __attribute__((ext_vector_type(2)));
template <int RB>
struct Chunk {  // widest power-of-two chunk (<= 16 B) that tiles a RB-byte row
  using t = typename std::conditional<RB % 16 == 0, f4v,
                                      typename std::conditional<RB % 8 == 0, f2v, float>::type>::type;
  static constexpr int N = RB / (int)sizeof(t);
};

// Action prefetch by LDS-DMA (global_load_lds_dword, non-temporal), issued from inline
// asm: the data lands in LDS without a VGPR destination and hipcc does not see the
// DMA at all -- so it neither drains vmcnt(0) before later LDS reads (its LDS-DMA
// alias rule) nor before reusing the address VGPRs, both of which it does for the
// builtin.  The loop waits explicitly with vmcnt(N), N = the vector-memory
// instructions it knows were issued after the DMA; older stores stay in flight.
// Destination = M0 (wave-uniform LDS byte offset) + lane * 4.
typedef __attribute__((address_space(3))) void* las_t;
__device__ __forceinline__ uint32_t lds_off(const float* p) {
  return (uint32_t)(uintptr_t)(las_t)(const_cast<float*>(p));
}
__device__ __forceinline__ void dma4_nt(const float* g, uint32_t m0) {
  uint32_t saved;  // M0 is a reserved register hipcc may hold a value in: save/restore
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\tglobal_load_lds_dword %1, off nt\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(saved)
               : "v"(g), "s"(m0)
               : "memory");
}
// 16-B LDS-DMA (global_load_lds_dwordx4); the s_nop separates the M0 write from the
// DMA that reads it.
__device__ __forceinline__ void dma16_nt(const float* g, uint32_t m0) {
  uint32_t saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(saved)
               : "v"(g), "s"(m0)
               : "memory");
}
// Row DMA of the fused rollout: ONE 16-B LDS-DMA per wave and step moves the wave's
// contiguous [envs, A] action slice (envs = 64, or 32 in the split-lane kernel) into the
// wave's own 1-KiB LDS region, row-major: lane l loads 16-B chunk l mod C of the slice
// (C = envs * A / 4 chunks; the remaining lanes repeat chunks, so no lane reads past
// the slice), landing at region + 16 l.  Needs the slice 16-B aligned (the launch's
// vec_ok: actions 16-B aligned, N a multiple of 4) and envs * A a multiple of 4.
template <int A, int E>
constexpr bool row_dma() { return (A == 2 || A == 3) && (E * A) % 4 == 0; }
constexpr int kRowRegionF = 256;  // floats per wave region and slot (64 lanes x 16 B)
// LDS floats of the DMA ring per slot for a B-lane workgroup
template <int A, int B>
constexpr int act_slot_floats() { return row_dma<A, 64>() ? (B / 64) * kRowRegionF : B * A; }
// LDS reads of the DMA'd slot, also from asm (with their own lgkmcnt wait), so that
// no compiler-visible LDS access depends on the hidden DMA.
template <int A>
__device__ __forceinline__ void lds_read_act(float* act, const float* p0, int stride) {
  if constexpr (A == 3) {
    asm volatile("ds_read_b32 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(act[0]), "=&v"(act[1]), "=&v"(act[2])
                 : "v"(lds_off(p0)), "v"(lds_off(p0 + stride)), "v"(lds_off(p0 + 2 * stride))
                 : "memory");
  } else {
    static_assert(A == 2, "action dim");
    asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(act[0]), "=&v"(act[1])
                 : "v"(lds_off(p0)), "v"(lds_off(p0 + stride))
                 : "memory");
  }
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt immediate (6 bits on gfx9)");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Prefetch distance D of the fused rollout's action DMA (steps in flight; D + 1 LDS
// slots, a power of two).  vmcnt counts stores as well as loads, so D also bounds how
// many steps of stores stay in flight behind the wait at the top of a step.
// D = 7 measured against 3 (tools/ab_rollout.py, K = 2048): LORENZ3 f32 +5% at 32,768
// envs (split lanes), +1.5% at 262,144; PMSM +4% at 32,768, even at 262,144.
constexpr int kDmaDist = 7;
template <int D>
constexpr int dma_slots() { return D + 1; }

// vmcnt wait at the top of step k < D: the vector-memory ops issued after step k's
// DMA are the prologue's later DMAs ((D-1-k) * kA) and k earlier steps' DMA + stores
template <int D, int kA, int kSt, int J = 0>
__device__ __forceinline__ void ladder_wait(int k) {
  if constexpr (J < D) {
    if (k == J) {
      wait_vmcnt<(D - 1 - J) * kA + J * (kA + kSt)>();
      return;
    }
    ladder_wait<D, kA, kSt, J + 1>(k);
  }
}

// ------------------------------------------------------------------ the ring
// How a wave's action slice of one step lies in its LDS slot:
//   Row     ONE 16-B DMA per wave and step, the slice row-major (row_dma above);
//   Direct  one 4-B DMA per component, component-major [A][B] (one-wave groups: every lane
//           DMAs its own env's components);
//   Staged  one 4-B DMA per component, a verbatim copy of the workgroup's row-major slice
//           (256-lane groups without row DMA).
enum class ActLayout { Row, Direct, Staged };

// The vmcnt accounting, stated once.  The DMA is invisible to hipcc (inline asm), so the
// loops wait for step k's actions themselves: s_waitcnt vmcnt(N) returns when at most N
// vector-memory instructions of the wave are outstanding, and they retire in order -- so
// N = the number of vector-memory instructions the wave ISSUED AFTER step k's DMA.  What
// is counted after a step's DMA: that step's stores (kSt: reward, done byte, obs chunks)
// and, for each of the D - 1 later steps already under way, its DMA (kA instructions) and
// its stores.  kSt is a LOWER bound on a step's stores: a wait with N smaller than the
// true count only waits for more than it needs (a few stores as well as the DMA), while
// an N that is too large would read the slot before its DMA has landed, with no error.
// Exec-masked stores (a dead lane's, the other half of a lane pair's) are still issued by
// the wave and still count -- the counts hold for ragged groups as long as one lane is
// live.  During the first D steps the prologue's later DMAs stand in for steps not yet
// run (ladder_wait); from step D on the count is the constant kSteady.
//
// A = action dim, E = envs per wave (64, or 32 with two lanes per env), B = workgroup
// lanes, D = prefetch distance (steps in flight; D + 1 slots), kSt_ = the loop's lower
// bound on its stores per step, L = the slot layout.
template <int A, int E, int B, int D, int kSt_, ActLayout L>
struct ActRing {
  static constexpr bool kRow = L == ActLayout::Row;
  static constexpr bool kDirect = L == ActLayout::Direct;
  static constexpr int kSt = kSt_;
  static constexpr int kA = kRow ? 1 : A;  // DMA instructions per step
  // steady-state wait: step k's DMA has one step's stores plus D-1 steps' (DMA +
  // stores) issued after it (lower bounds, see kSt)
  static constexpr int kSteady = kSt + (D - 1) * (kA + kSt);
  static_assert(D >= 1 && kSteady <= 63, "vmcnt immediate (6 bits on gfx9)");
  static constexpr int kDmaSlots = dma_slots<D>();
  static constexpr int kSlotF = kRow ? (B / 64) * kRowRegionF : B * A;  // LDS floats per slot
  static constexpr int kChunks = A > 0 ? E * A / 4 : 1;  // Row: 16-B chunks of a wave's slice

  // M0 = LDS byte address of this wave's 64 destination floats: computed once,
  // wave-uniform, then constant offsets per slot / component (no per-DMA address-space
  // cast or readfirstlane)
  static __device__ __forceinline__ uint32_t wave_m0(const float* s_act, int wave) {
    return __builtin_amdgcn_readfirstlane(lds_off(s_act) + (uint32_t)wave * (kRow ? kRowRegionF * 4u : 256u));
  }
  // DMA one step's action slice into LDS slot `slot`; src = this lane's first source
  // float of that step (component j is j, resp. j*B, on)
  static __device__ __forceinline__ void issue(const float* src, uint32_t m0_wave, int slot) {
    if constexpr (kRow) {
      dma16_nt(src, m0_wave + (uint32_t)(slot * kSlotF) * 4u);
    } else {
#pragma unroll
      for (int j = 0; j < A; ++j)
        dma4_nt(src + (kDirect ? j : j * B), m0_wave + (uint32_t)((slot * A + j) * B) * 4u);
    }
  }
  // The lane's DMA source within its wave's / group's slice: Row -- the 16-B chunk lane l
  // loads (chunk l mod C); else -- the env row whose components it loads.  kRag (the
  // ragged last group on the full path): clamped to the group's own nb rows (nb * A
  // floats, whole 16-B chunks since nb % 4 == 0), so no lane reads past the slice
  template <bool kRag>
  static __device__ __forceinline__ int src_chunk(int lane, int nb) {
    return kRag ? min(lane % kChunks, nb * A / 4 - 1) : lane % kChunks;
  }
  template <bool kRag>
  static __device__ __forceinline__ int src_row(int row, int nb) {
    return kRag ? min(row, nb - 1) : row;
  }
  // The D-deep prologue fill: step d's slice into slot d, near the end step K-1 again (no
  // branch, same op count).  Returns the running source of the DMA issued at step k (step
  // min(k + D, K - 1)), advanced by one step per step until it reaches the last (no
  // per-step 64-bit multiply).  lane0 = the lane's first source float of step 0.
  // (K by reference: every use reads the launch argument where a written-out loop does --
  // passed by value, the one early read reorders the prologue of every action kernel.
  // split_loop keeps its own fill written out: called there, this function changes the
  // code of one kernel, k_rollout_pair at D = 15.)
  static __device__ __forceinline__ const float* fill(const float* gact, int64_t lane0, int64_t dstride,
                                                      const int32_t& K, uint32_t m0_wave) {
#pragma unroll
    for (int d = 0; d < D; ++d) issue(gact + ((int64_t)(d < K ? d : K - 1) * dstride + lane0), m0_wave, d);
    return gact + ((int64_t)(D < K ? D : K - 1) * dstride + lane0);
  }
  // The wait for step k's actions.  kLadder: one of the first D steps (its wait count
  // depends on k); later steps all wait with the steady-state count -- peeled so the hot
  // loop carries no ladder
  template <bool kLadder>
  static __device__ __forceinline__ void wait(int k) {
    if constexpr (kLadder) ladder_wait<D, kA, kSt>(k);
    else wait_vmcnt<kSteady>();
  }
  static __device__ __forceinline__ const float* slot(const float* s_act, int k) {
    return s_act + (k % kDmaSlots) * kSlotF;
  }
  // prefetch step k+D into the slot step k-1 used (every reader is past this point);
  // near the end re-read step K-1: no branch, same op count
  static __device__ __forceinline__ void refill(const float*& dsrc, int64_t dstride, int k, int K,
                                                uint32_t m0_wave) {
    issue(dsrc, m0_wave, (k + D) % kDmaSlots);
    if (k + D + 1 < K) dsrc += dstride;
  }
};

// The ragged path's action row (a ragged last group / unaligned actions): each lane loads
// its own row, ONE STEP AHEAD into registers (a load issued and waited for in the same
// step put a memory round trip into every step of the group's chain: PMSM 24,608 x 2048,
// one ragged group of 32 envs, 3,421 us against 2,094 at 24,576, profiles/r06/pair/).
// act = step k's row, anext = step k+1's on return; off = k * n.
template <int A>
__device__ __forceinline__ void act_row_ahead(float* act, float* anext, const float* gact, int64_t i,
                                              int64_t off, int64_t n, int k, int K) {
  if (k == 0) {
#pragma unroll
    for (int j = 0; j < A; ++j) anext[j] = gload<true>(gact + i * A + j);
  }
#pragma unroll
  for (int j = 0; j < A; ++j) act[j] = anext[j];
  if (k + 1 < K) {
#pragma unroll
    for (int j = 0; j < A; ++j) anext[j] = gload<true>(gact + (off + n + i) * A + j);
  }
}

}  // namespace lz
