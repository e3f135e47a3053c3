// The one list of systems: which launcher key runs which Sys type (lz_systems.h), whether
// a float64 instantiation exists, and which policy rollouts are built for it.  Every host
// launcher (lz_kernels.hip, lz_policy.hip) and the host-side SysInfo (lz_internal.h) go
// through for_system(); a system added here is added everywhere, and a launcher that names
// a policy family the entry does not list does not compile a kernel for it.
#pragma once
#include <type_traits>

#include "lz_internal.h"
#include "lz_systems.h"

namespace lz {

// What for_system() hands its callable: the Sys instantiation and its scalar type.
// policies (kPol* of lz_internal.h) is empty for a float64 tag: the policy rollouts are
// float32 only.
template <class S, typename Scalar, unsigned kPolicies, bool kHasF64>
struct SysTag {
  using Sys = S;
  using T = Scalar;
  static constexpr unsigned policies = kPolicies;
  static constexpr bool has_f64 = kHasF64;
  static constexpr bool runs(PolicyKind k) { return (kPolicies & pol_bit(k)) != 0; }
};

template <template <typename> class S, bool kF64, unsigned kPolicies, class Fn>
inline int visit_system(bool f64, Fn& fn) {
  if constexpr (kF64) {
    if (f64) return fn(SysTag<S<double>, double, 0u, kF64>{});
  }
  return fn(SysTag<S<float>, float, kPolicies, kF64>{});
}
template <typename>
using SysPMSMf = SysPMSM;  // float32 only: the reference computes it in float32

// fn(SysTag) for the launcher key `system` (lz_config.system, + kSysRK4 for the RK4
// integrator mode) and dtype; hipErrorInvalidValue for an unknown key.  A plain switch
// over a generic callable: nothing here allocates or calls through a pointer.  Per entry:
// the Sys template, whether float64 is built, the policy rollouts built (kPolEval /
// kPolEvalAttn: the fused evaluation of the float32 MlpPolicy / attention actor-critics).
template <class Fn>
inline int for_system(int system, bool f64, Fn&& fn) {
  switch (system) {
    case LZ_SYS_LORENZ3: return visit_system<SysL3, true, kPolAll | kPolMlpI8 | kPolEval | kPolEvalAttn | kPolMlpStack>(f64, fn);
    case LZ_SYS_LORENZ4: return visit_system<SysL4, true, kPolBasic | kPolMlpI8 | kPolEval>(f64, fn);
    case LZ_SYS_LORENZ3 + kSysRK4: return visit_system<SysL3RK4, true, 0u>(f64, fn);
    case LZ_SYS_LORENZ4 + kSysRK4: return visit_system<SysL4RK4, true, 0u>(f64, fn);
    case LZ_SYS_PMSM: return visit_system<SysPMSMf, false, kPolAll | kPolMlpI8 | kPolEval | kPolEvalAttn | kPolMlpStack>(f64, fn);
    case LZ_SYS_HR: return visit_system<SysHR, true, kPolAll | kPolMlpI8 | kPolEval | kPolEvalAttn | kPolMlpStack>(f64, fn);
    case LZ_SYS_T1: return visit_system<SysT1, true, kPolBasic>(f64, fn);
    case LZ_SYS_T2: return visit_system<SysT2, true, kPolBasic>(f64, fn);
    case LZ_SYS_TP: return visit_system<SysTP, true, kPolBasic>(f64, fn);
    case LZ_SYS_SC: return visit_system<SysSC, true, kPolBasic>(f64, fn);
  }
  return (int)hipErrorInvalidValue;
}

// The host-side facts of a tag's system, read off its Sys type.
template <class Tag>
constexpr SysInfo sys_info_of() {
  using Sys = typename Tag::Sys;
  static_assert(Sys::n_planes == Sys::kStepPlane + 1 && Sys::n_planes <= kMaxPlanes, "step plane is the last");
  return {Sys::state_dim, Sys::A,          Sys::O,           Sys::NI,      Sys::n_planes, Sys::kStepPlane,
          Sys::t_planes,  Sys::kUsesAction, Sys::kNoise,     Tag::has_f64, Tag::policies};
}

}  // namespace lz
