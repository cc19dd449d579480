// sqrt_cert_gpu.hip -- sgk_sqrt_cert (sigtk_amd/csrc/tstat_math.h) on the GPU, with the hardware's v_rsq_f32, over the
// floats of a file: what store_event_fast (csrc/event_build.h) computes for an event's standard deviation.
//   tools/sqrt_cert_gpu IN OUT     IN: n float32; OUT: n x {uint32 bits of the certified form, uint32 bits of the
//                                  final value (the certified form, or sqrtf where it is not certified), uint32 ok}
// Build (sigtk_amd/build.py: build_tools): the library's numerics flags, -ffp-contract=off and correctly rounded sqrt.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../sigtk_amd/csrc/tstat_math.h"

__global__ void k(const float *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = in[i];
    bool dom_ok, cert_ok;
    const float s = sgk_sqrt_cert(v, dom_ok, cert_ok);
    const bool ok = dom_ok & cert_ok;
    float r = s;
    if (!ok) {
        __asm__ volatile("" ::: "memory");
        r = sqrtf(v);
    }
    out[3 * i] = __float_as_uint(s);
    out[3 * i + 1] = __float_as_uint(r);
    out[3 * i + 2] = ok ? 1u : 0u;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const uint32_t n = (uint32_t)(bytes / 4);
    std::vector<float> h(n ? n : 1);
    if (n && fread(h.data(), 4, n, f) != n) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    std::vector<uint32_t> o(3 * (size_t)(n ? n : 1));
    if (n) {
        float *din; uint32_t *dout;
        CHECK(hipMalloc(&din, (size_t)n * 4));
        CHECK(hipMalloc(&dout, (size_t)n * 12));
        CHECK(hipMemcpy(din, h.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(o.data(), dout, (size_t)n * 12, hipMemcpyDeviceToHost));
        CHECK(hipFree(din));
        CHECK(hipFree(dout));
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (n && fwrite(o.data(), 12, n, f) != n) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    return 0;
}
