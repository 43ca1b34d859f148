// store_policy.h -- cache policy of the stores that hand a training step's buffers from one kernel to the next (gfx950).
//
// The four kernels of a step (k_encode_tiles -> k_fused_train<PRE> -> k_grid_scatter -> k_optimizer) talk through global memory only, and the kernel
// boundary is the only synchronisation: the eight XCDs' L2s are not coherent with each other, so whatever a kernel leaves dirty in its L2 is written back
// before the next one starts.  A store's policy decides WHEN its bytes leave the L2, never what they are:
//   plain  : write-back; the line stays dirty in the XCD's L2 until it is evicted or the end-of-kernel release writes it back
//   nt     : non-temporal (streaming) hint, still write-back
//   wt     : write-through (the sc1 bit): the bytes go out as the store retires, nothing of them is left for the boundary
//   wt_nt  : both bits
// Every buffer has ONE compile-time policy (MON_SP_<buffer>), overridable with -D for A/B libraries (tools/variant_build.sh <tag> -DMON_SP_E=MON_SP_WT ...);
// -DMON_SP_HANDOVER=<policy> sets every hand-over buffer at once and -DMON_SP_ALL=<policy> the optimizer state as well (MON_SP_ALL=MON_SP_PLAIN is the
// library without any policy).  The product reads no environment variable for this: a policy is a fact of the build.
// Consumers need nothing: the next launch's acquire invalidates its caches as it always did.  Measurements: profiles/r10_store_policy.md.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define MON_SP_PLAIN 0
#define MON_SP_NT 1
#define MON_SP_WT 2
#define MON_SP_WT_NT 3

// ---- the policies in force.  MON_SP_DEFAULT(d): the shipped policy d of a hand-over buffer unless a variant build overrides the whole set.
#if defined(MON_SP_ALL)
#define MON_SP_DEFAULT(d) MON_SP_ALL
#elif defined(MON_SP_HANDOVER)
#define MON_SP_DEFAULT(d) MON_SP_HANDOVER
#else
#define MON_SP_DEFAULT(d) d
#endif
#ifndef MON_SP_E            // k_encode_tiles: encoded features E[L][B] half2 (4 B per lane, during the last walk)
#define MON_SP_E MON_SP_DEFAULT(MON_SP_WT)
#endif
#ifndef MON_SP_DE           // k_fused_train: dL/dE rows de_soa[L][B] half2 (4 B per lane, at the end of each ray)
#define MON_SP_DE MON_SP_DEFAULT(MON_SP_WT)
#endif
#ifndef MON_SP_XSOA         // k_fused_train: positions of the gradient-carrying samples x_soa[B] float4 (16 B)
#define MON_SP_XSOA MON_SP_DEFAULT(MON_SP_WT)
#endif
#ifndef MON_SP_DW           // k_fused_train: one fp32 dW partial row per workgroup (16 B, the kernel's last phase)
#define MON_SP_DW MON_SP_DEFAULT(MON_SP_WT)
#endif
#ifndef MON_SP_RAYOUT       // k_fused_train: per-ray colour / depth / mask / loss (4 B from one lane per ray)
#define MON_SP_RAYOUT MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_GPART        // k_grid_scatter: fp16 partial tables (4 / 8 / 16 B, the tile write-out)
#define MON_SP_GPART MON_SP_DEFAULT(MON_SP_WT)
#endif
#ifndef MON_SP_HALF         // k_optimizer: fp16 working copy (16 B)
#define MON_SP_HALF MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_TILES        // k_optimizer: the fp16 grid in tile order for k_encode_tiles (16 / 8 B)
#define MON_SP_TILES MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_EMA          // k_optimizer: EMA shadow copy (16 B)
#define MON_SP_EMA MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_XALL         // position blocks (k_optimizer, k_sample_points): x_all[B] float4 and the ray records (16 B)
#define MON_SP_XALL MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_FRAG         // k_optimizer: MFMA A-fragment image of the MLP weights (2 B)
#define MON_SP_FRAG MON_SP_DEFAULT(MON_SP_PLAIN)
#endif
#ifndef MON_SP_STATE        // k_optimizer: master weights, Adam moments, step counters (16 B; small tables only, see kernels_optim.hip)
#ifdef MON_SP_ALL
#define MON_SP_STATE MON_SP_ALL
#else
#define MON_SP_STATE MON_SP_NT
#endif
#endif

namespace mon {

// One store of 2, 4, 8 or 16 bytes per lane with policy POLICY.  Vector stores only.  The write-through forms: a relaxed agent-scope atomic store up to 8 B
// (the compiler emits the global store with sc1 and keeps counting it), inline assembly where no such form exists (16 B; both bits together).  The assembly
// forms carry no memory clobber -- they are for buffers the storing kernel does not read back -- and end in the wait states the data registers need before
// the compiler may reuse them.
template <int POLICY, class T> __device__ __forceinline__ void policy_store(T v, T* p) {
    static_assert(sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "policy_store: 2, 4, 8 or 16 bytes per lane");
    static_assert(POLICY >= MON_SP_PLAIN && POLICY <= MON_SP_WT_NT, "policy_store: unknown policy");
    typedef uint32_t sp_u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) uint16_t* sp_g16; typedef __attribute__((address_space(1))) uint32_t* sp_g32;
    typedef __attribute__((address_space(1))) unsigned long long* sp_g64;
    if constexpr (POLICY == MON_SP_PLAIN) *p = v;
    else if constexpr (POLICY == MON_SP_NT) {
        if constexpr (sizeof(T) == 2) __builtin_nontemporal_store(__builtin_bit_cast(uint16_t, v), reinterpret_cast<uint16_t*>(p));
        else if constexpr (sizeof(T) == 4) __builtin_nontemporal_store(__builtin_bit_cast(uint32_t, v), reinterpret_cast<uint32_t*>(p));
        else if constexpr (sizeof(T) == 8) __builtin_nontemporal_store(__builtin_bit_cast(unsigned long long, v), reinterpret_cast<unsigned long long*>(p));
        else __builtin_nontemporal_store(__builtin_bit_cast(sp_u32x4, v), reinterpret_cast<sp_u32x4*>(p));
    } else if constexpr (POLICY == MON_SP_WT) {
        if constexpr (sizeof(T) == 2) __hip_atomic_store((sp_g16)(uintptr_t)p, __builtin_bit_cast(uint16_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if constexpr (sizeof(T) == 4) __hip_atomic_store((sp_g32)(uintptr_t)p, __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if constexpr (sizeof(T) == 8)
            __hip_atomic_store((sp_g64)(uintptr_t)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(__builtin_bit_cast(sp_u32x4, v)));
    } else {
        if constexpr (sizeof(T) == 2) asm volatile("global_store_short %0, %1, off sc1 nt\n\ts_nop 1" :: "v"(p), "v"((uint32_t)__builtin_bit_cast(uint16_t, v)));
        else if constexpr (sizeof(T) == 4) asm volatile("global_store_dword %0, %1, off sc1 nt\n\ts_nop 1" :: "v"(p), "v"(__builtin_bit_cast(uint32_t, v)));
        else if constexpr (sizeof(T) == 8)
            asm volatile("global_store_dwordx2 %0, %1, off sc1 nt\n\ts_nop 1" :: "v"(p), "v"(__builtin_bit_cast(unsigned long long, v)));
        else asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" :: "v"(p), "v"(__builtin_bit_cast(sp_u32x4, v)));
    }
}

}  // namespace mon
