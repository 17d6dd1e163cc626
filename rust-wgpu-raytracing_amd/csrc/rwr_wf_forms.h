// How the wavefront integrator's launchers pick a kernel (kernels_wf_primary.hip, kernels_wf_bounce.hip, kernels_wf_shadow.hip).
//
// A FORM of a kernel template is the tuple of its template arguments, packed into a small integer.  Beside each template sits
// a description F of its forms:
//   F::Form                the template's arguments, by name
//   F::kRange              forms are numbered 0 .. kRange - 1
//   F::encode, F::decode   Form <-> number
//   F::valid(Form)         which forms exist — the one place that says so
//   F::Kernel              the pointer type all instantiations share
//   F::kernel<I>()         &k<decode(I)...>
// and the template's FORM TABLE, form_table<F>(): entry I is F::kernel<I>() when decode(I) is valid and null otherwise, built
// at compile time, so every valid form is instantiated by the table and no other is.  A launcher computes the form from what
// the frame needs and launches through the table: hipLaunchKernelGGL(table[F::encode({...})], grid, block, lds, stream, args...).
// check_forms<F>(n) — a static_assert beside each table — says that decode and encode agree and how many forms there are.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <initializer_list>
#include <utility>

namespace rwr {

template <class F, uint32_t I>
constexpr typename F::Kernel form_kernel()
{
    if constexpr (F::valid(F::decode(I))) return F::template kernel<I>();   // (an invalid form is never instantiated)
    else return nullptr;
}
template <class F, size_t... I>
constexpr std::array<typename F::Kernel, sizeof...(I)> form_table(std::index_sequence<I...>)
{
    return {{form_kernel<F, (uint32_t)I>()...}};
}
template <class F>
constexpr auto form_table() { return form_table<F>(std::make_index_sequence<F::kRange>{}); }

// how many valid forms `pred` holds for
template <class F>
constexpr uint32_t count_forms(bool (*pred)(typename F::Form) = nullptr)
{
    uint32_t n = 0;
    for (uint32_t i = 0; i < F::kRange; i++)
        if (F::valid(F::decode(i)) && (!pred || pred(F::decode(i)))) n++;
    return n;
}
// every valid form's number decodes and encodes to itself, and there are n_valid of them
template <class F>
constexpr bool check_forms(uint32_t n_valid)
{
    for (uint32_t i = 0; i < F::kRange; i++)
        if (F::valid(F::decode(i)) && F::encode(F::decode(i)) != i) return false;
    return count_forms<F>() == n_valid;
}

// A kernel whose dynamic LDS goes beyond the default limit of 64 KiB.  A function attribute belongs to the function ON ONE
// DEVICE: raised once per device a context renders on (raised_on: one bit per device), for all of `kernels` together.
template <class Kernel>
hipError_t raise_dynamic_lds_once(std::atomic<uint64_t> &raised_on, int bytes, std::initializer_list<Kernel> kernels)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (raised_on.load(std::memory_order_acquire) & bit) return hipSuccess;
    for (Kernel k : kernels) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    raised_on.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

}  // namespace rwr
