// Host-side helpers shared by the translation units of libfarnn_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include "common.hip.h"

namespace farnn {

inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// Switches a create call refuses instead of ignoring (include/farnn.h): forms that live in the A/B build only, asked of the
// production library, and switches of earlier rounds that no longer exist.  Checked where the switches are read: once per
// handle, in farnn_*_create / farnn_train_create -- never on the tagging path.
inline int check_env_switches() {
#if !defined(FARNN_AB)
    for (const char *name : {"FARNN_CV_ONE", "FARNN_CV_STASH", "FARNN_NODEST"})
        if (env_int(name, 0))
            return fail(FARNN_EINVAL, "%s is set: that form is compiled into the A/B build only (csrc/build.py --probes; load it with "
                                      "FARNN_LIB=.../libfarnn_hip_probes.so)%s", name);
#endif
    for (const char *name : {"FARNN_CV_WIDE", "FARNN_DECOMP_OLD"})
        if (env_int(name, 0))
            return fail(FARNN_EINVAL, "%s is set: that switch was removed (round 5; include/farnn.h lists the supported ones)%s", name);
    return FARNN_OK;
}

// first step of every farnn_*_create / farnn_train_create: refuse unsupported switches, then make `device` current
inline int select_device(int device) {
    if (int rc = check_env_switches()) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(FARNN_ENODEV, "no HIP device visible%s%s");
    if (device < 0 || device >= n) return fail(FARNN_EINVAL, "device index out of range%s%s");
    FARNN_HIP_TRY(hipSetDevice(device));
    return FARNN_OK;
}

// ---- the FARNN_* environment switches -------------------------------------------------------------------------------
// Every switch the library knows, read ONCE per handle when it is created (farnn_*_create / farnn_train_create): no call on
// the tagging path touches the environment.  SUPPORTED switches (include/farnn.h lists them) select between code paths the
// test suite holds to the same results; DIAGNOSTIC ones (ablations, geometry overrides of the tuning scripts) exist in the
// profiling build only (build.py --probes, -DFARNN_PROBES) -- the production library ignores them.
#define FARNN_TUNABLES(X)                                                                                      \
    /* supported */                                                                                            \
    X(NOFUSE, 0, true) X(FUSE, 0, true) X(NOREGS, 0, true) X(NOLABELMAP, 0, true) X(PREP, 0, true) X(NOSORT, 0, true)           \
    X(VITERBI_BP, 0, true) X(VITERBI_UNFUSED, 0, true) X(DECOMP_NOREGS, 0, true)                               \
    X(ROWS_NOREGS, 0, true) X(TRAIN_NOLDS, 0, true) X(TRAIN_NSEQ, 0, true)              \
    X(WIDE_UNPAIRED, 0, true) X(ROWS_LPR4, 0, true) X(ROWS_NOROUNDS, 0, true) X(NOHALF, 0, true)                  \
    /* A/B build only (the production library refuses them at create: check_env_switches) */                   \
    X(CV_ONE, 0, false) X(CV_STASH, 0, false) X(NODEST, 0, false)                                              \
    /* diagnostic: profiling build only */                                                                     \
    X(DBG, 0, false) X(KS, 3, false) X(RPG, 12, false) X(NLD, 4, false) X(NOFAST, 0, false)                    \
    X(CHAIN_HELPER, 0, false) X(HOST_EPOCH, 0, false) X(CV_NOSORT, 0, false) X(NOKZ, 0, false)                 \
    X(FUSE_SPIN, 4, false) X(SOLO_MARGIN, 24, false) X(DECOMP_FOUR, 0, false) X(ROWS_NSEQ, 0, false)
enum TunId {
#define FARNN_TUN_ENUM(name, dflt, prod) TUN_##name,
    FARNN_TUNABLES(FARNN_TUN_ENUM)
#undef FARNN_TUN_ENUM
    TUN_COUNT
};
struct Tunables {
    int v[TUN_COUNT];
    Tunables() {
#if defined(FARNN_PROBES)
        constexpr bool diag = true;
#else
        constexpr bool diag = false;
#endif
#define FARNN_TUN_READ(name, dflt, prod) v[TUN_##name] = ((prod) || diag) ? env_int("FARNN_" #name, dflt) : (dflt);
        FARNN_TUNABLES(FARNN_TUN_READ)
#undef FARNN_TUN_READ
    }
};
// the handle the current C-ABI call works for: tun(TUN_X) reads ITS snapshot (one caller thread per handle, include/farnn.h)
extern thread_local const Tunables *g_tun;
struct TunScope {
    const Tunables *prev;
    explicit TunScope(const Tunables *t) : prev(g_tun) { g_tun = t; }
    ~TunScope() { g_tun = prev; }
};
inline int tun(TunId id) {
    static const Tunables defaults_at_load;              // (outside any handle's call: the environment as the library was loaded)
    return (g_tun ? g_tun : &defaults_at_load)->v[id];
}

// The refusal of a launch whose dynamic LDS cannot fit a workgroup (pure: a step can ask before it enqueues anything)
inline int lds_fits(size_t bytes) {
    return bytes > 160 * 1024 ? fail(FARNN_ERANGE, "kernel needs more than 160 KiB of LDS%s%s") : FARNN_OK;
}

// Raise a kernel's dynamic-LDS limit (needed above 48 KiB).  The attribute is sticky, so it is set
// only when a kernel needs more than it was last given (a host API call per launch otherwise).
template <typename KernelT>
inline int raise_lds_limit(KernelT kern, size_t bytes) {
    static std::map<std::pair<int, const void *>, size_t> granted;    // (device, kernel) -> bytes
    static std::mutex granted_mu;                                     // (handles on different threads share the map)
    if (int rc = lds_fits(bytes)) return rc;
    if (bytes <= 48 * 1024) return FARNN_OK;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const void *fn = reinterpret_cast<const void *>(kern);
    std::lock_guard<std::mutex> lock(granted_mu);
    size_t &g = granted[{dev, fn}];
    if (bytes > g) {
        FARNN_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        g = bytes;
    }
    return FARNN_OK;
}

// The one way a kernel with dynamic LDS is launched: raise its LDS limit if it needs that, then enqueue it (the kernel is named once).
template <typename... Params, typename... Args>
inline int launch(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args &&...args) {
    if (int rc = raise_lds_limit(kern, lds)) return rc;
    kern<<<grid, block, lds, s>>>(std::forward<Args>(args)...);
    return FARNN_OK;
}
// The same with the event pair of a timer that rides on the kernel's own dispatch packet (both null: a plain launch).
template <typename... Params, typename... Args>
inline int launch_timed(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                        Args &&...args) {
    if (int rc = raise_lds_limit(kern, lds)) return rc;
    if (e0 && e1) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, s, e0, e1, 0, std::forward<Args>(args)...);
    else kern<<<grid, block, lds, s>>>(std::forward<Args>(args)...);
    return FARNN_OK;
}
template <int N>
using int_c = std::integral_constant<int, N>;
inline int device_cus(int device) {      // compute units (256 if the device does not say)
    int ncu = 0;
    return hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0 ? ncu : 256;
}

// A device buffer that only grows.  A too-small one is freed after a device synchronize (an earlier step's kernels may still
// use it).  `what` is the message of a failed allocation: it names the step and the buffer, and holds two "%s" (fail()); `a` fills
// the first (a step's prefix, where the message is shared by several steps).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    int ensure(size_t need, const char *what, const char *a = "") {
        if (need <= n) return FARNN_OK;
        if (p) { FARNN_HIP_TRY(hipDeviceSynchronize()); release(); }
        if (hipMalloc((void **)&p, need * sizeof(T)) != hipSuccess) { p = nullptr; return fail(FARNN_ENOMEM, what, a); }
        n = need;
        return FARNN_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

}  // namespace farnn
