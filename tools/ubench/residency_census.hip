// Census: how many 256-thread workgroups of the resting frame kernel's resources does one CU hold at once?
// (DESIGN.md §4.1 "Lean resting form".)  Four kernels whose code objects report 64 VGPRs and
// {94, 80} SGPRs (.sgpr_count) x {18 432, 4 096} B of LDS — a clobbered high register and a dummy __shared__ array, nothing
// else.  Every workgroup stamps the 100 MHz clock at its start and end, sleeps a fixed, counted time in between (about 40 us)
// and leaves the stamps with its XCC and CU ids; the host counts, per CU, the most workgroups alive at one instant.
//   hipcc --offload-arch=gfx950 -O3 residency_census.hip -o residency_census && ./residency_census
// (-Rpass-analysis=kernel-resource-usage shows the four resource lines.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define CHECK(x)                                                                                      \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));        \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

struct Stamp { unsigned long long t0, t1; uint32_t xcc, hw_id; };

// HIGH_SGPR: true clobbers s87 (next free 88, .sgpr_count 94), false s73 (74 / 80).  LDS_BYTES: the dummy array.
template <bool HIGH_SGPR, uint32_t LDS_BYTES>
__global__ void __launch_bounds__(256) k_census(Stamp *out, uint32_t sleeps)
{
    __shared__ uint32_t s_dummy[LDS_BYTES / 4u];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    if (HIGH_SGPR) asm volatile("" ::: "s87");
    else asm volatile("" ::: "s73");
    asm volatile("" ::: "v63");
    s_dummy[threadIdx.x] = threadIdx.x;
    for (uint32_t i = 0; i < sleeps; i++) __builtin_amdgcn_s_sleep(127);   // 127 x 64 cycles each; counted, so bounded
    __syncthreads();   // the stamp below is the workgroup's end, not the first wave's
    if (threadIdx.x == 0u) {
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        Stamp st;
        st.t0 = t0;
        st.t1 = __builtin_amdgcn_s_memrealtime();
        st.xcc = (xcc & 0xfu) | (s_dummy[255] == 255u ? 0u : 0x80000000u);   // (keeps the array)
        st.hw_id = hw;
        out[blockIdx.x] = st;
    }
}

template <bool HIGH_SGPR, uint32_t LDS_BYTES>
static int census(const char *name, Stamp *d_out, uint32_t n_wg, uint32_t sleeps)
{
    int api = 0;
    hipFuncAttributes fa;
    CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_census<HIGH_SGPR, LDS_BYTES>)));
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, k_census<HIGH_SGPR, LDS_BYTES>, 256, 0));
    CHECK(hipMemset(d_out, 0, n_wg * sizeof(Stamp)));
    hipLaunchKernelGGL((k_census<HIGH_SGPR, LDS_BYTES>), dim3(n_wg), dim3(256), 0, 0, d_out, sleeps);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<Stamp> h(n_wg);
    CHECK(hipMemcpy(h.data(), d_out, n_wg * sizeof(Stamp), hipMemcpyDeviceToHost));
    // per CU (XCC, then the SE / SH / CU fields of HW_ID: bits 8-15): +1 at a start, -1 at an end, ends first at equal stamps
    std::map<uint32_t, std::vector<std::pair<unsigned long long, int>>> per_cu;
    unsigned long long life = 0;
    for (const Stamp &s : h) {
        const uint32_t cu = (s.xcc & 0xfu) << 8 | ((s.hw_id >> 8) & 0xffu);
        per_cu[cu].push_back({s.t0, +1});
        per_cu[cu].push_back({s.t1, -1});
        life += s.t1 - s.t0;
    }
    std::map<int, int> hist;
    int most = 0;
    for (auto &kv : per_cu) {
        std::sort(kv.second.begin(), kv.second.end());   // (-1 sorts ahead of +1)
        int alive = 0, top = 0;
        for (auto &ev : kv.second) { alive += ev.second; top = std::max(top, alive); }
        hist[top]++;
        most = std::max(most, top);
    }
    printf("%-26s vgpr %3d  lds %6zu B  api %d  CUs seen %3zu  mean life %.1f us  most alive on a CU %d  (CUs by their most:", name, fa.numRegs,
           fa.sharedSizeBytes, api, per_cu.size(), (double)life / n_wg / 100.0, most);
    for (auto &kv : hist) printf(" %d:%d", kv.first, kv.second);
    printf(")\n");
    return 0;
}

int main()
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const uint32_t n_wg = (uint32_t)prop.multiProcessorCount * 8u * 4u, sleeps = 12u;
    Stamp *d_out = nullptr;
    CHECK(hipMalloc(&d_out, n_wg * sizeof(Stamp)));
    printf("# %s, %d CUs, %u workgroups of 256 threads, %u x s_sleep 127 each\n", prop.name, prop.multiProcessorCount, n_wg, sleeps);
    for (int pass = 0; pass < 2; pass++) {   // (the second pass runs on a clocked-up chip with the code loaded)
        if (census<true, 18432u>("sgpr 94, lds 18432", d_out, n_wg, sleeps)) return 1;
        if (census<false, 18432u>("sgpr 80, lds 18432", d_out, n_wg, sleeps)) return 1;
        if (census<true, 4096u>("sgpr 94, lds  4096", d_out, n_wg, sleeps)) return 1;
        if (census<false, 4096u>("sgpr 80, lds  4096", d_out, n_wg, sleeps)) return 1;
    }
    CHECK(hipFree(d_out));
    return 0;
}
