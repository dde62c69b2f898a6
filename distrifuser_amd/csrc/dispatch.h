// Host-side launcher helpers: a runtime dtype or bool becomes a template
// argument of a generic lambda, so a launcher names its kernel and arguments
// once:
//
//   dispatch_dtype(dtype, [&]<typename T>(std::type_identity<T>) {
//       dispatch_bool(silu, [&]<bool SILU>(std::bool_constant<SILU>) {
//           kernel<T, SILU><<<grid, block, 0, stream>>>((const T*)x, ...);
//       });
//   });
#pragma once

#include "common.h"
#include "kernels.h"
#include <algorithm>
#include <type_traits>

// bf16 / fp16 element type; anything else is fp32
template <typename F>
void dispatch_dtype(int dtype, F&& f) {
    switch (dtype) {
        case DFA_BF16: f(std::type_identity<bf16_t>{}); break;
        case DFA_F16: f(std::type_identity<f16_t>{}); break;
        default: f(std::type_identity<float>{}); break;
    }
}

// the F16 axis of the 16-bit kernels; anything but DFA_F16 is bf16
template <typename F>
void dispatch_f16(int dtype, F&& f) {
    if (dtype == DFA_F16)
        f(std::true_type{});
    else
        f(std::false_type{});
}

template <typename F>
void dispatch_bool(bool v, F&& f) {
    if (v)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// blocks of a grid-stride elementwise launch
inline int grid_for(int64_t work, int block) {
    return (int)std::min<int64_t>((work + block - 1) / block, 4096);
}
