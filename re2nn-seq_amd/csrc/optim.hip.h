// The multi-tensor optimizer step (farnn_optim_*; include/farnn.h): Adam (torch.optim.Adam's defaults: no
// weight decay, no amsgrad) and plain SGD over every tensor of a training step in ONE launch.
//
// The tensors are cut into chunks of OPT_CHUNK elements at create; the chunk table (tensor, offset, count) lives on the device
// and never changes.  What changes from step to step -- the pointers and each tensor's bias corrections -- travels as the
// kernel's argument (OptArgs: OPT_MAX_TENSORS tensors per launch; a longer list takes more launches).  One workgroup updates
// one chunk: a pure stream (Adam reads param, grad and both moments and writes param and both moments: 7 x 4 bytes per
// element), no LDS, no atomics, nothing carried between elements.  With 16 bytes per lane and OPT_CHUNK / (4 x OPT_THREADS) = 2
// such accesses per lane and array, a workgroup keeps 32 KiB of loads in flight and needs about 40 registers: eight of them
// fit a compute unit, which is more than the memory system needs to stay busy (MI355X: a streaming kernel is bound by HBM
// once every unit has a few tens of KiB in flight).  A chunk whose pointers are not all 16-byte aligned (a view that starts
// inside a storage) goes element by element, and so do the last count % 4 elements of a tensor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace farnn {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 2048;            // elements per workgroup: a multiple of 4 x OPT_THREADS
constexpr int OPT_MAX_TENSORS = 32;        // tensors per launch (the kernel's argument holds their pointers: 1.4 KiB)
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a full chunk is a whole number of 16-byte accesses per lane");

struct OptChunk {
    int32_t tensor;                        // index into OptArgs of the launch this chunk belongs to
    int32_t count;                         // 1..OPT_CHUNK elements
    int64_t off;                           // first element: a multiple of OPT_CHUNK
};

struct OptArgs {
    float *p[OPT_MAX_TENSORS];
    const float *g[OPT_MAX_TENSORS];       // null: the tensor has no gradient in this step and is left alone
    float *m[OPT_MAX_TENSORS], *v[OPT_MAX_TENSORS];      // exp_avg, exp_avg_sq (Adam)
    float step_size[OPT_MAX_TENSORS];      // Adam: lr / (1 - beta1^t), t the tensor's own step count; SGD: lr
    float bc2_sqrt[OPT_MAX_TENSORS];       // Adam: sqrt(1 - beta2^t)
    float w1, beta2, w2, eps;              // 1 - beta1, beta2, 1 - beta2, eps
};

// torch.optim.Adam, one element: exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2);
// param.addcdiv_(exp_avg, exp_avg_sq.sqrt() / sqrt(bc2) + eps, value = -lr / bc1)
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, float step_size, float bc2_sqrt,
                                             float w1, float beta2, float w2, float eps) {
    m = m + (g - m) * w1;
    v = v * beta2 + w2 * g * g;
    p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
}

template <bool ADAM>
__global__ void __launch_bounds__(OPT_THREADS) optim_step_kernel(const OptChunk *__restrict__ chunks, OptArgs a) {
    const OptChunk c = chunks[blockIdx.x];
    const int t = c.tensor;
    const float *gb = a.g[t];
    if (!gb) return;                       // (uniform: the whole workgroup leaves)
    float *p = a.p[t] + c.off;
    const float *g = gb + c.off;
    float *m = ADAM ? a.m[t] + c.off : nullptr, *v = ADAM ? a.v[t] + c.off : nullptr;
    const float step_size = a.step_size[t], bc2_sqrt = a.bc2_sqrt[t];
    const float w1 = a.w1, beta2 = a.beta2, w2 = a.w2, eps = a.eps;
    const int n = c.count;
    uintptr_t bits = (uintptr_t)p | (uintptr_t)g;
    if (ADAM) bits |= (uintptr_t)m | (uintptr_t)v;
    const int nvec = (bits & 15) ? 0 : n >> 2;           // 16-byte accesses of this chunk
    constexpr int PER = OPT_CHUNK / (4 * OPT_THREADS);
    if (nvec == OPT_CHUNK / 4) {                         // a full aligned chunk: every load issued before the first use
        float4 P[PER], G[PER], M[PER], V[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = k * OPT_THREADS + threadIdx.x;
            P[k] = reinterpret_cast<const float4 *>(p)[i];
            G[k] = reinterpret_cast<const float4 *>(g)[i];
            if (ADAM) { M[k] = reinterpret_cast<const float4 *>(m)[i]; V[k] = reinterpret_cast<const float4 *>(v)[i]; }
        }
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = k * OPT_THREADS + threadIdx.x;
            if (ADAM) {
                adam_element(P[k].x, G[k].x, M[k].x, V[k].x, step_size, bc2_sqrt, w1, beta2, w2, eps);
                adam_element(P[k].y, G[k].y, M[k].y, V[k].y, step_size, bc2_sqrt, w1, beta2, w2, eps);
                adam_element(P[k].z, G[k].z, M[k].z, V[k].z, step_size, bc2_sqrt, w1, beta2, w2, eps);
                adam_element(P[k].w, G[k].w, M[k].w, V[k].w, step_size, bc2_sqrt, w1, beta2, w2, eps);
                reinterpret_cast<float4 *>(m)[i] = M[k];
                reinterpret_cast<float4 *>(v)[i] = V[k];
            } else {
                P[k].x -= step_size * G[k].x; P[k].y -= step_size * G[k].y;
                P[k].z -= step_size * G[k].z; P[k].w -= step_size * G[k].w;
            }
            reinterpret_cast<float4 *>(p)[i] = P[k];
        }
        return;
    }
    for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {      // the last chunk of a tensor
        float4 P = reinterpret_cast<const float4 *>(p)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        if (ADAM) {
            float4 M = reinterpret_cast<const float4 *>(m)[i], V = reinterpret_cast<const float4 *>(v)[i];
            adam_element(P.x, G.x, M.x, V.x, step_size, bc2_sqrt, w1, beta2, w2, eps);
            adam_element(P.y, G.y, M.y, V.y, step_size, bc2_sqrt, w1, beta2, w2, eps);
            adam_element(P.z, G.z, M.z, V.z, step_size, bc2_sqrt, w1, beta2, w2, eps);
            adam_element(P.w, G.w, M.w, V.w, step_size, bc2_sqrt, w1, beta2, w2, eps);
            reinterpret_cast<float4 *>(m)[i] = M;
            reinterpret_cast<float4 *>(v)[i] = V;
        } else {
            P.x -= step_size * G.x; P.y -= step_size * G.y; P.z -= step_size * G.z; P.w -= step_size * G.w;
        }
        reinterpret_cast<float4 *>(p)[i] = P;
    }
    for (int i = 4 * nvec + threadIdx.x; i < n; i += OPT_THREADS) {   // the tail, or a chunk that is not 16-byte aligned
        float P = p[i];
        const float G = g[i];
        if (ADAM) {
            float M = m[i], V = v[i];
            adam_element(P, G, M, V, step_size, bc2_sqrt, w1, beta2, w2, eps);
            m[i] = M; v[i] = V;
        } else {
            P -= step_size * G;
        }
        p[i] = P;
    }
}

}  // namespace farnn
