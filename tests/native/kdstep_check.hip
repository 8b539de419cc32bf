// GPU known-answer harness for the two short forms of one kd decision (csrc/device_math.hpp kd_below and
// div_by_rcp_wave_bounded, used by csrc/traverse.hpp kd_step).  Built once and run by tests/test_gpu_kdstep.py:
//   kdstep_check <in.bin> <out.bin>
// in.bin: records of 5 little-endian 32-bit words (floats as their bit patterns), one case per lane:
//   oa, split, da        kd_below's inputs as the step has them
//   a, b                 the division's dividend and divisor; its reciprocal is rcp_for_div(b), as trav_begin's
// out.bin: 3 words per case: kd_below(split - oa, da) as 0 / 1; div_by_rcp_wave_bounded(a, b, rcp_for_div(b));
//   div_by_rcp_wave of the same.
// The cases run in blocks of 64 (one wave each), so a wave's mix of lanes inside and outside the short
// division's range is the test's choice; a trailing partial wave runs with its other lanes inactive.
// Nothing is compared here: every expected value is computed on the host by the test.  One JSON line to stdout.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "device_math.hpp"

using namespace cr;

enum { KD_IN = 5, KD_OUT = 3 };

__global__ void k_kdstep(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *c = in + (size_t)KD_IN * i;
    uint32_t *o = out + (size_t)KD_OUT * i;
    const float oa = __uint_as_float(c[0]), split = __uint_as_float(c[1]), da = __uint_as_float(c[2]);
    o[0] = kd_below(split - oa, da) ? 1u : 0u;
    const float a = __uint_as_float(c[3]), b = __uint_as_float(c[4]);
    const float y = rcp_for_div(b);
    o[1] = __float_as_uint(div_by_rcp_wave_bounded(a, b, y));
    o[2] = __float_as_uint(div_by_rcp_wave(a, b, y));
}

#define HIP_OK(x)                                                                                                      \
    do {                                                                                                               \
        const hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "kdstep_check: %s: %s\n", #x, hipGetErrorString(e_));                                      \
            return 2;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: kdstep_check <in.bin> <out.bin>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (4 * KD_IN)) {
        fclose(f);
        fprintf(stderr, "kdstep_check: input is not a whole number of records\n");
        return 2;
    }
    std::vector<uint32_t> in((size_t)bytes / 4);
    const bool read_ok = fread(in.data(), 4, in.size(), f) == in.size();
    fclose(f);
    if (!read_ok) return 2;
    const uint32_t n = (uint32_t)(in.size() / KD_IN);
    std::vector<uint32_t> out((size_t)n * KD_OUT, 0u);
    if (n) {
        uint32_t *di = nullptr, *dout = nullptr;
        HIP_OK(hipMalloc(&di, in.size() * 4));
        HIP_OK(hipMalloc(&dout, out.size() * 4));
        HIP_OK(hipMemcpy(di, in.data(), in.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0, out.size() * 4));
        hipLaunchKernelGGL(k_kdstep, dim3((n + 63) / 64), dim3(64), 0, 0, di, dout, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
        (void)hipFree(di);
        (void)hipFree(dout);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) return 2;
    printf("{\"cases\": %u}\n", n);
    return 0;
}
