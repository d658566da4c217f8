// tr8_probe — pins the lane layout of ds_read_b64_tr_b8 that attn_mfma_f8.h relies on (gfx950).
// An LDS image of 32 rows x 16 bytes is read twice, once holding every byte's row and once its column. Every lane of
// group g = lane / 16 supplies the address of row 8 g + (lane % 16) / 2, columns 8 (lane % 2) .. +7. Expected: lane
// 16 g + i holds column i of rows 8 g .. 8 g + 7, row 8 g + q in its byte q.
// Prints every lane's 8 bytes as (row, column) pairs and PASS / FAIL (exit status 0 / 1).
//   hipcc --offload-arch=gfx950 -O2 tools/tr8_probe.hip -o tools/tr8_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

__global__ void probe(uint2* out) {
    __shared__ __attribute__((aligned(16))) unsigned char img[32 * 16];
    const int lane = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        for (int i = lane; i < 32 * 16; i += 64) img[i] = (unsigned char)(pass == 0 ? i / 16 : i % 16);
        __syncthreads();
        const int g = lane >> 4, i16 = lane & 15;
        const unsigned addr = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)img +
                              (unsigned)((8 * g + (i16 >> 1)) * 16 + 8 * (i16 & 1));
        uint2 v;
        asm volatile("ds_read_b64_tr_b8 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
        out[pass * 64 + lane] = v;
    }
}

int main() {
    uint2* d = nullptr;
    if (hipMalloc(&d, 128 * sizeof(uint2)) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    uint2 h[128];
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const unsigned long long rows = ((unsigned long long)h[lane].y << 32) | h[lane].x;
        const unsigned long long cols = ((unsigned long long)h[64 + lane].y << 32) | h[64 + lane].x;
        printf("lane %2d:", lane);
        for (int q = 0; q < 8; ++q) {
            const int r = (int)((rows >> (8 * q)) & 0xFF), c = (int)((cols >> (8 * q)) & 0xFF);
            printf(" (%2d,%2d)", r, c);
            if (r != 8 * (lane >> 4) + q || c != (lane & 15)) ++bad;
        }
        printf("\n");
    }
    printf("%s: %d bytes differ from 'lane 16 g + i holds column i of rows 8 g .. 8 g + 7, row 8 g + q in byte q'\n",
           bad ? "FAIL" : "PASS", bad);
    (void)hipFree(d);
    return bad ? 1 : 0;
}
