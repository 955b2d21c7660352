// The floor of a DEPENDENT launch of the label-map score kernel's grid (K2l, csrc/score_decode.hip.h): what one more kernel of
// 256 workgroups x W wavefronts costs behind a recurrence-sized kernel on the same stream when it does nothing at all -- the
// launch, the dispatch of its wavefronts and the end-of-kernel hand-over, without a single load.  Whatever K2l takes above this is
// the kernel's own dependent chain; whatever it takes below cannot be had without removing the launch.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/probe/empty_launch.hip -o /tmp/empty_launch && /tmp/empty_launch
//
// The kernel in front stands in for K1d: 512 workgroups of 512 threads that wait ~25 us on the wall clock.  Per W in {4, 8, 16}:
// HIP events around `reps` x (front) and around `reps` x (front, empty<W>), alternated `rounds` times; the floor is the difference
// of the per-step means.  The empty kernel takes an argument block of the size of K2l's (ScoreParams: ~220 bytes).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct Args { long long words[28]; };

__global__ void __launch_bounds__(512) front_kernel(long long ticks, long long *sink) {
    // wall_clock64: the 100 MHz constant clock
    const long long t0 = wall_clock64();
    long long t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (sink && t == 0) *sink = t;
}

template <int W>
__global__ void __launch_bounds__(W * 64) empty_kernel(const Args a) {
    if (a.words[0] == 0x7fffffffffffffffll) reinterpret_cast<long long *>(a.words[1])[0] = 0;      // never: keeps the argument live
}

template <int W>
static float run(int reps, bool with_empty, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Args &a) {
    CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < reps; i++) {
        front_kernel<<<512, 512, 0, s>>>(2500, nullptr);
        if (with_empty) empty_kernel<W><<<256, W * 64, 0, s>>>(a);
    }
    CHECK(hipEventRecord(e1, s));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1000.0f / reps;
}

template <int W>
static void measure(int reps, int rounds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    Args a = {};
    std::vector<float> base, both;
    run<W>(reps, true, s, e0, e1, a);                     // warm-up
    for (int r = 0; r < rounds; r++) {
        base.push_back(run<W>(reps, false, s, e0, e1, a));
        both.push_back(run<W>(reps, true, s, e0, e1, a));
    }
    std::sort(base.begin(), base.end());
    std::sort(both.begin(), both.end());
    const float mb = base[rounds / 2], mw = both[rounds / 2];
    printf("empty<<<256, %2d x 64>>> behind a 25 us kernel: front alone %.2f us (min %.2f max %.2f), with the empty launch %.2f us "
           "(min %.2f max %.2f): floor %.2f us per step\n", W, mb, base.front(), base.back(), mw, both.front(), both.back(), mw - mb);
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200, rounds = argc > 2 ? atoi(argv[2]) : 7;
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    measure<4>(reps, rounds, s, e0, e1);
    measure<8>(reps, rounds, s, e0, e1);
    measure<16>(reps, rounds, s, e0, e1);
    CHECK(hipStreamSynchronize(s));
    return 0;
}
