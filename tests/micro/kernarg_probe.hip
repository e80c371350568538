// Micro-benchmark (diagnostic, not product): what one kernarg round trip costs at the front of a
// launch in a captured chain of dependent launches, and whether the box's firmware preloads kernel
// arguments into SGPRs.  Build twice from this one source:
//   hipcc --offload-arch=gfx950 -O3 kernarg_probe.hip -o kernarg_probe_sload
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 kernarg_probe.hip -o kernarg_probe_preload
// The kernel takes seven pointer/size scalars (14 dwords: what the preload covers) and then a
// 256-byte by-value struct, like the decode kernels' leading scalars + mv_args, and does ONE global
// load whose address needs only the scalars; the struct is read after it.  A graph of NODES such
// launches, each reading what the previous wrote, is replayed with a kernel in between that streams
// a buffer larger than the Infinity Cache, so the kernarg lines are cold as in a decode step.
// Each chain is measured twice: with bare nodes (the launch itself is all there is), and with every
// node held for `delay` sleeps after its load (about a decode kernel's length), which leaves the
// command processor the previous node's run time to fetch the next node's arguments.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));  \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

struct tail_args {  // 256 bytes, by value, behind the scalars
    float add;
    int delay;  // s_sleep(64) repeats after the load: the node's length without any memory traffic
    long long pad[31];
};
static_assert(sizeof(tail_args) == 256, "256-byte struct");

constexpr int GRID = 256, NTH = 64, NODES = 92;

// n = GRID * NTH elements per buffer; every index is clamped to [0, n)
__global__ void __launch_bounds__(NTH) k_link(const float *src, float *dst, const float *bias, long long n,
                                              long long stride, long long off, long long bias_n, tail_args t) {
    long long i = ((long long)blockIdx.x * NTH + threadIdx.x) * stride + off;
    i = i < n ? i : n - 1;
    const float v = src[i];  // the one dependent load: its address needs src, n, stride, off only
    for (int k = 0; k < t.delay; ++k) __builtin_amdgcn_s_sleep(64);
    long long j = (long long)blockIdx.x * NTH + threadIdx.x;
    j = j < n ? j : n - 1;
    dst[j] = v + t.add + bias[j < bias_n ? j : bias_n - 1];
}

__global__ void __launch_bounds__(256) k_stream(const uint4 *buf, long long n16, unsigned *sink) {
    unsigned acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
        const uint4 v = buf[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 30;
    const int delay = argc > 2 ? atoi(argv[2]) : 2;
    const long long n = (long long)GRID * NTH;
    float *buf[2], *bias;
    CHECK(hipMalloc(&buf[0], n * 4));
    CHECK(hipMalloc(&buf[1], n * 4));
    CHECK(hipMalloc(&bias, n * 4));
    CHECK(hipMemset(buf[0], 0, n * 4));
    CHECK(hipMemset(buf[1], 0, n * 4));
    CHECK(hipMemset(bias, 0, n * 4));
    const long long big = 1024ll << 20;  // 1 GiB: four times the 256 MiB Infinity Cache
    uint4 *cold;
    unsigned *sink;
    CHECK(hipMalloc(&cold, big));
    CHECK(hipMalloc(&sink, 4));
    CHECK(hipMemset(cold, 1, big));
    hipStream_t s;
    CHECK(hipStreamCreate(&s));
    tail_args t = {};
    t.add = 1.0f;

    long long launched = 0;
    for (int held = 0; held < 2; ++held) {
        t.delay = held ? delay : 0;
        hipGraph_t g;
        hipGraphExec_t ge;
        CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
        for (int k = 0; k < NODES; ++k)
            hipLaunchKernelGGL(k_link, dim3(GRID), dim3(NTH), 0, s, buf[k & 1], buf[(k + 1) & 1], bias, n, 1ll, 0ll, n, t);
        CHECK(hipStreamEndCapture(s, &g));
        CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));

        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        for (int cold_run = 1; cold_run >= 0; --cold_run) {
            std::vector<float> us;
            for (int r = 0; r < reps + 3; ++r) {
                if (cold_run) hipLaunchKernelGGL(k_stream, dim3(2048), dim3(256), 0, s, cold, big / 16, sink);
                CHECK(hipEventRecord(e0, s));
                CHECK(hipGraphLaunch(ge, s));
                CHECK(hipEventRecord(e1, s));
                CHECK(hipStreamSynchronize(s));
                float ms;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 3) us.push_back(ms * 1000.0f / NODES);
            }
            std::sort(us.begin(), us.end());
            launched += (long long)(reps + 3) * NODES;
            printf("%s %s replays=%d nodes=%d us/launch min %.3f median %.3f max %.3f\n", held ? "held " : "bare ", cold_run ? "cold(streamed 1 GiB before)" : "warm(back to back)",
                   reps, NODES, us.front(), us[us.size() / 2], us.back());
        }
        CHECK(hipGraphExecDestroy(ge));
        CHECK(hipGraphDestroy(g));
    }
    float h;
    CHECK(hipMemcpy(&h, buf[0], 4, hipMemcpyDeviceToHost));  // NODES even: the last node wrote buf[0]
    printf("check: buf[0][0] = %.0f (expect %.0f)\n", h, (float)launched);
    return 0;
}
