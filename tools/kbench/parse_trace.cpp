// Developer micro-benchmark for the parse render kernel (not part of the product; built and run by hand on the GPU box):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DAIR_TRACE tools/kbench/parse_trace.cpp -o tools/kbench/bin/parse_trace
//   tools/kbench/bin/parse_trace [images=65536] [T=3] [H=W=50] [h=w=20] [present steps per image: -1 = r mod (T + 1)]
// Includes the kernel translation unit directly, so the kernel measured is the shipped one; with -DAIR_TRACE thread 0 of every
// workgroup stamps the chip-wide 100 MHz counter at the phase boundaries marked AIR_TR(i) in parse_render_kernel.  A workgroup of a
// grid-stride launch overwrites its stamps unit by unit: what is read back are the phases of each workgroup's LAST unit.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "../../attend_infer_repeat_amd/csrc/parse_kernels.hip"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

static float frand() { return (float)rand() / (float)RAND_MAX; }
template <typename T> static T *dev(const std::vector<T> &v) {
    T *p; CK(hipMalloc(&p, v.size() * sizeof(T))); CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); return p;
}

int main(int argc, char **argv) {
    const int R = argc > 1 ? atoi(argv[1]) : 65536, T = argc > 2 ? atoi(argv[2]) : 3;
    const int H = argc > 3 ? atoi(argv[3]) : 50, W = H, h = argc > 4 ? atoi(argv[4]) : 20, w = h;
    const int fixed = argc > 5 ? atoi(argv[5]) : -1;
    const size_t M = (size_t)T * R, HW = (size_t)H * W, hw = (size_t)h * w;
    srand(1);
    std::vector<float> where(M * 4), glm(M * hw), pres(M), obs((size_t)R * HW);
    for (size_t k = 0; k < M; ++k) {
        where[4 * k] = 0.3f + 0.4f * frand(); where[4 * k + 1] = 0.6f * frand() - 0.3f;
        where[4 * k + 2] = 0.3f + 0.4f * frand(); where[4 * k + 3] = 0.6f * frand() - 0.3f;
    }
    for (auto &x : glm) x = frand() - 0.5f;
    for (auto &x : obs) x = frand();
    for (int t = 0; t < T; ++t)
        for (int r = 0; r < R; ++r) pres[(size_t)t * R + r] = t < (fixed >= 0 ? fixed : r % (T + 1)) ? 1.f : 0.f;
    float *d_where = dev(where), *d_glm = dev(glm), *d_pres = dev(pres), *d_obs = dev(obs), *d_rec, *d_parts;
    signed char *d_owner; int *d_area;
    int NB, RB;                                                    // air_canvas_unroll_bands' rule (that entry lives in canvas_kernels.hip)
    { int nb = 256 / (R < 1 ? 1 : R); if (nb > 8) nb = 8; wr_bands(H, nb, &NB, &RB); }
    CK(hipMalloc(&d_rec, (size_t)R * HW * 4)); CK(hipMalloc(&d_parts, (size_t)NB * R * 4)); CK(hipMalloc(&d_owner, (size_t)R * HW));
    CK(hipMalloc(&d_area, M * 4));
    hipStream_t st; CK(hipStreamCreate(&st));
    auto run = [&](bool with_rec) {
        int rc = air_parse_render(d_glm, d_where, d_pres, with_rec ? d_obs : nullptr, 0.5f, 0.3f, 0.02f, T, R, H, W, h, w, NB, d_rec,
                                  with_rec ? d_parts : nullptr, d_owner, d_area, nullptr, st);
        if (rc) { printf("air_parse_render returned %d\n", rc); exit(1); }
    };
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    for (int with_rec = 1; with_rec >= 0; --with_rec) {
        for (int i = 0; i < 5; ++i) run(with_rec);
        std::vector<double> reps;
        for (int rep = 0; rep < 5; ++rep) {
            CK(hipEventRecord(a, st));
            for (int i = 0; i < 10; ++i) run(with_rec);
            CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b)); reps.push_back(ms * 100.0);
        }
        std::sort(reps.begin(), reps.end());
        printf("images=%d T=%d %dx%d glimpse %dx%d bands=%d present=%d rec=%d: %.1f us/launch (median of 5 x 10)\n", R, T, H, W, h, w, NB,
               fixed, with_rec, reps[2]);
#ifdef AIR_TRACE
        std::vector<unsigned long long> tr(AIR_TRACE_BLOCKS * AIR_TRACE_PHASES);
        CK(hipMemcpyFromSymbol(tr.data(), HIP_SYMBOL(air_trace), tr.size() * 8));
        const char *names[4] = {"loads issued, staging + tables written", "barrier (waits for the loads)", "pixel pass", "counts, reconstruction sum, area"};
        for (int ph = 0; ph < 4; ++ph) {
            double sum = 0; int cnt = 0;
            for (int g = 0; g < AIR_TRACE_BLOCKS; ++g) {
                const unsigned long long t0 = tr[g * AIR_TRACE_PHASES + ph], t1 = tr[g * AIR_TRACE_PHASES + ph + 1];
                if (t0 && t1) { sum += (double)(t1 - t0); ++cnt; }
            }
            if (cnt) printf("   phase %d -> %d  %-42s mean %6.2f us per unit (%d workgroups' last unit)\n", ph, ph + 1, names[ph], sum / cnt * 0.01, cnt);
        }
#endif
    }
    return 0;
}
