#pragma once
// dispatch.cuh — host side: runtime values -> kernel template arguments.  Each helper
// calls the generic lambda f with std::integral_constant tags and returns what f returns;
// in the lambda a tag's value is decltype(TAG)::value (usable in nested lambdas too).  A
// launch site names its kernel and writes its argument list once:
//   with_act(act, [&](auto A) {
//     with_vec_nt(vec, nt, [&](auto V, auto N) {
//       hipLaunchKernelGGL((k<decltype(V)::value, decltype(N)::value, decltype(A)::value>), grid, block, 0, st, ...);
//     });
//   });
// Only the listed values are instantiated: a site gets exactly the kernels it names.
#include <type_traits>

#include "vsiq_common.cuh"

namespace vsiq {

template <bool B>
using BoolC = std::bool_constant<B>;
template <int V>
using IntC = std::integral_constant<int, V>;

template <class F>
decltype(auto) with_bool(bool b, F &&f) {
  return b ? f(BoolC<true>{}) : f(BoolC<false>{});
}

// f(BoolC<a>, BoolC<b>): all four combinations (codes x mask, ...)
template <class F>
decltype(auto) with_bool2(bool a, bool b, F &&f) {
  return a ? (b ? f(BoolC<true>{}, BoolC<true>{}) : f(BoolC<true>{}, BoolC<false>{}))
           : (b ? f(BoolC<false>{}, BoolC<true>{}) : f(BoolC<false>{}, BoolC<false>{}));
}

// the first listed value equal to v, else the last listed
template <int V0, int... Vs, class F>
decltype(auto) with_int(int v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) return f(IntC<V0>{});
  else return v == V0 ? f(IntC<V0>{}) : with_int<Vs...>(v, f);
}

// the first listed value >= v (ascending list), else the last listed
template <int V0, int... Vs, class F>
decltype(auto) with_int_le(int64_t v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) return f(IntC<V0>{});
  else return v <= V0 ? f(IntC<V0>{}) : with_int_le<Vs...>(v, f);
}

// the activation kind of a C ABI act argument: relu, silu, else none
template <class F>
decltype(auto) with_act(int act, F &&f) {
  const int k = act_kind(act);
  return k == kActRelu ? f(IntC<kActRelu>{}) : k == kActSilu ? f(IntC<kActSilu>{}) : f(IntC<kActNone>{});
}

// the element type of a C ABI dtype argument (VSIQ_DT_*; dtype_ok checked it): f(TypeC<T>),
// T = typename decltype(D)::type.  A site's 16-bit cases call functions that are explicitly
// instantiated in the 16-bit translation units (k_*_half.hip), so the fp32 objects hold
// fp32 kernels only.
template <class T>
struct TypeC {
  using type = T;
};
inline bool dtype_ok(int dtype) { return dtype == VSIQ_DT_F32 || dtype == VSIQ_DT_BF16 || dtype == VSIQ_DT_F16; }

template <class F>
decltype(auto) with_dtype(int dtype, F &&f) {
  return dtype == VSIQ_DT_BF16 ? f(TypeC<bf16_t>{}) : dtype == VSIQ_DT_F16 ? f(TypeC<f16_t>{}) : f(TypeC<float>{});
}

// f(VEC, NT) over (1,1), (1,0), (0,0): the scalar path has no non-temporal instance
template <class F>
decltype(auto) with_vec_nt(bool vec, bool nt, F &&f) {
  return vec && nt ? f(BoolC<true>{}, BoolC<true>{}) : vec ? f(BoolC<true>{}, BoolC<false>{})
                                                            : f(BoolC<false>{}, BoolC<false>{});
}

// f(VEC, NT) over all four pairs
template <class F>
decltype(auto) with_vec_nt4(bool vec, bool nt, F &&f) {
  return with_bool2(vec, nt, f);
}

}  // namespace vsiq
