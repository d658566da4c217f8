// bgemm_mx8_lab.hip — diagnostic: the block-scaled batched decode projection (csrc/bgemm_mx8.h) on the five C4 launches
// (Llama-3-8B shapes: q/k/v, wo, gate/up, down, LM head) under every forced plan (tpw, splits, wt, wk) of a grid, each
// timed over NL distinct weight images inside a replayed hipGraph (no Infinity-Cache re-reads), the store epilogue
// throughout (norm as the launch has it). Prints per launch every plan's us and GB/s of weight bytes, the fastest, the
// planner's pick (bg_mx8_plan) and its distance from the fastest, and for both the per-workgroup stamps (s_memrealtime,
// 10 ns ticks): mean us from entry to the staged image, through the stream, through the epilogue.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include tools/bgemm_mx8_lab.hip -o tools/bgemm_mx8_lab
//   tools/bgemm_mx8_lab [batch] > profiles/bgemm_mx8_lab.txt
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simplellminference_amd/csrc/bgemm_mx8.h"

using namespace sli;

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

// image bytes: any codes; scale bytes 119 .. 134, so that no sum overflows
__global__ void fill_b(uint8_t* p, size_t n, unsigned seed, int scales) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u ^ seed;
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        p[i] = scales ? (uint8_t)(119 + (h & 15)) : (uint8_t)h;
    }
}
__global__ void fill_f(float* p, size_t n, unsigned seed, float off) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2246822519u ^ seed;
        h ^= h >> 13;
        h *= 2654435761u;
        h ^= h >> 16;
        p[i] = off + (float)(h & 0xFFFF) / 65536.0f - 0.5f;
    }
}

struct Bufs {
    std::vector<uint8_t*> W, S;
    float *x, *nw, *y, *ws;
    unsigned* cnt;
    unsigned long long* stamps;
};

static Bg8Plan make_plan(int ntiles, int K, int tpw, int s, int wk) {
    Bg8Plan p;
    p.ntiles = ntiles;
    p.tpw = tpw;
    p.splits = s;
    p.wk = wk;
    p.wt = kBgWaves / wk;
    p.groups = (ntiles + tpw - 1) / tpw;
    p.lds = bg8_lds_bytes(K, s, tpw, wk);
    return p;
}

static Bg8In make_in(const Bufs& b, int K, int B, bool norm, int i) {
    Bg8In in{};
    in.x = b.x;
    in.norm_w = norm ? b.nw : nullptr;
    in.eps = 1e-5f;
    in.K = K;
    in.B = B;
    in.ws = b.ws;
    in.counters = b.cnt;
    in.tiled = 1;
    in.w = b.W[i];
    in.wscale = b.S[i];
    return in;
}

static double time_plan(const Bufs& b, int rows, int K, int B, bool norm, const Bg8Plan& p, int reps) {
    hipStream_t s;
    CK(hipStreamCreate(&s));
    const BgEpiStore e{b.y, nullptr, nullptr, 1.0f, rows, rows};
    const int NL = (int)b.W.size();
    for (int i = 0; i < NL; ++i) CK(launch_bgemm_mx8(make_in(b, K, B, norm, i), e, p, s));  // warm-up
    CK(hipStreamSynchronize(s));
    hipGraph_t g;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    for (int i = 0; i < NL; ++i) CK(launch_bgemm_mx8(make_in(b, K, B, norm, i), e, p, s));
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    CK(hipGraphLaunch(ge, s));
    CK(hipStreamSynchronize(s));
    hipEvent_t a, z;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&z));
    CK(hipEventRecord(a, s));
    for (int r = 0; r < reps; ++r) CK(hipGraphLaunch(ge, s));
    CK(hipEventRecord(z, s));
    CK(hipEventSynchronize(z));
    float ms;
    CK(hipEventElapsedTime(&ms, a, z));
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(z));
    CK(hipGraphExecDestroy(ge));
    CK(hipGraphDestroy(g));
    CK(hipStreamDestroy(s));
    return 1000.0 * ms / (reps * (double)NL);
}

// one stamped launch: mean over the workgroups of the three phases, and the launch's span (first entry to last end)
static void stamps(const Bufs& b, int rows, int K, int B, bool norm, const Bg8Plan& p, const char* tag) {
    const int wgs = p.groups * p.splits;
    const BgEpiStore e{b.y, nullptr, nullptr, 1.0f, rows, rows};
    Bg8In in = make_in(b, K, B, norm, 0);
    in.stamps = b.stamps;
    CK(hipMemset(b.stamps, 0, sizeof(unsigned long long) * 4 * wgs));
    CK(launch_bgemm_mx8(in, e, p, nullptr));
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(4 * (size_t)wgs);
    CK(hipMemcpy(h.data(), b.stamps, h.size() * 8, hipMemcpyDeviceToHost));
    double st = 0, sm = 0, ep = 0;
    unsigned long long lo = ~0ull, hi = 0;
    int ends = 0;  // with splits only a group's last arriver runs the epilogue and writes the fourth stamp
    for (int w = 0; w < wgs; ++w) {
        const unsigned long long* t = &h[4 * (size_t)w];
        st += (double)(t[1] - t[0]);
        sm += (double)(t[2] - t[1]);
        lo = std::min(lo, t[0]);
        hi = std::max(hi, t[2]);
        if (t[3]) {
            ep += (double)(t[3] - t[2]);
            hi = std::max(hi, t[3]);
            ++ends;
        }
    }
    const double u = 0.01 / wgs;  // 100 MHz ticks -> us, mean
    printf("    stamps %-8s mean per workgroup: stage+quantise %.2f us, stream %.2f us, epilogue / publish+merge %.2f us (%d of %d workgroups); "
           "first entry to last end %.2f us\n",
           tag, st * u, sm * u, ep * 0.01 / std::max(ends, 1), ends, wgs, (double)(hi - lo) * 0.01);
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 8;
    struct Shape { const char* name; int rows, K; bool norm; };
    const Shape shapes[] = {{"qkv", 6144, 4096, true}, {"wo", 4096, 4096, false}, {"gate_up", 28672, 4096, true},
                            {"down", 4096, 14336, false}, {"lm_head", 128256, 4096, true}};
    const int tpws[] = {1, 2, 3, 4, 6, 7, 8, 12, 16, 24, 32, 48, 64};
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    Bufs b;
    CK(hipMalloc(&b.x, sizeof(float) * 8 * 16384));
    CK(hipMalloc(&b.nw, sizeof(float) * 16384));
    CK(hipMalloc(&b.y, sizeof(float) * 8 * 131072));
    CK(hipMalloc(&b.ws, 256 << 20));
    CK(hipMalloc(&b.cnt, 1 << 20));
    CK(hipMemset(b.cnt, 0, 1 << 20));
    CK(hipMalloc(&b.stamps, 8 * 4 * 65536));
    fill_f<<<256, 256>>>(b.x, 8 * 16384, 3, 0.0f);
    fill_f<<<256, 256>>>(b.nw, 16384, 5, 1.0f);
    CK((bg8_allow_lds<BgEpiStore, true>()));
    CK((bg8_allow_lds<BgEpiStore, false>()));
    printf("bgemm_mx8_lab: batch %d, %d CUs, ring %d; us per launch over rotated weight images in a replayed graph\n", B, cus, kBg8Ring);
    for (const Shape& sh : shapes) {
        const int ntiles = (sh.rows + 15) / 16;
        const size_t db = bg_tiled_mx_bytes(ntiles, sh.K), sb = bg_tiled_mx_scale_bytes(ntiles, sh.K);
        // rotate at least 600 MB (more than the 256 MB Infinity Cache holds), 3 to 64 images
        const int NL = (int)std::max<size_t>(3, std::min<size_t>(64, ((size_t)600 << 20) / db + 1));
        b.W.assign(NL, nullptr);
        b.S.assign(NL, nullptr);
        for (int i = 0; i < NL; ++i) {
            CK(hipMalloc(&b.W[i], db));
            CK(hipMalloc(&b.S[i], sb));
            fill_b<<<1024, 256>>>(b.W[i], db, 11 + i, 0);
            fill_b<<<256, 256>>>(b.S[i], sb, 23 + i, 1);
        }
        CK(hipDeviceSynchronize());
        const double bytes = (double)db + (double)sb;
        printf("%s: %d x %d, norm %d, %d tiles, %d weight images of %.1f MB\n", sh.name, sh.rows, sh.K, (int)sh.norm, ntiles, NL, bytes / 1e6);
        double best = 1e30;
        Bg8Plan bp;
        for (int s : {1, 2, 4, 8})
            for (int wk = 1; wk <= 16; wk *= 2)
                for (int tpw : tpws) {
                    if (sh.norm && s > 1) continue;
                    if (bg8_plan_refusal(ntiles, sh.K, sh.norm, tpw, s, 16 / wk, wk)) continue;
                    const Bg8Plan p = make_plan(ntiles, sh.K, tpw, s, wk);
                    const int wgs = p.groups * s;
                    if (wgs < cus / 4 || wgs > 8 * cus || tpw > ntiles) continue;  // neither a quarter-empty chip nor 8 passes
                    if ((size_t)p.ntiles * s * 512 > ((size_t)256 << 20) || p.groups > (1 << 18)) continue;
                    const double us = time_plan(b, sh.rows, sh.K, B, sh.norm, p, 5);
                    printf("  tpw %2d splits %d wt %2d x wk %2d  wgs %5d  %8.2f us  %7.1f GB/s\n", tpw, s, p.wt, wk, wgs, us, bytes / us / 1e3);
                    if (us < best) best = us, bp = p;
                }
        const Bg8Plan pp = bg_mx8_plan(ntiles, sh.K, B, sh.norm, cus);
        const double pus = time_plan(b, sh.rows, sh.K, B, sh.norm, pp, 10), bus = time_plan(b, sh.rows, sh.K, B, sh.norm, bp, 10);
        printf("  fastest: tpw %d splits %d wt %d x wk %d  %.2f us (%.1f GB/s)\n", bp.tpw, bp.splits, bp.wt, bp.wk, bus, bytes / bus / 1e3);
        printf("  planner: tpw %d splits %d wt %d x wk %d  %.2f us (%.1f GB/s), %.3f of the fastest\n", pp.tpw, pp.splits, pp.wt, pp.wk, pus,
               bytes / pus / 1e3, pus / bus);
        stamps(b, sh.rows, sh.K, B, sh.norm, bp, "fastest");
        stamps(b, sh.rows, sh.K, B, sh.norm, pp, "planner");
        for (int i = 0; i < NL; ++i) {
            CK(hipFree(b.W[i]));
            CK(hipFree(b.S[i]));
        }
    }
    return 0;
}
