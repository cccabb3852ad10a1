// lr_accum.h -- the host scaffold the accumulators of kept draws share (lr_predict, lr_acf, lr_marg, lr_loo in lr_api.hip): a grow-only
// device workspace, the loop that cuts one accumulate call into staged pieces, and the small helpers around them.  What differs between
// accumulators stays with each: its struct, the argument checks of its create call, its launch, result and reset functions.
// Host code only; included by lr_api.hip alone, after lr_model.h (fail, LR_HIP, lr_model, LR_BY_DTYPE) and lr_predict.h (k_predict_pad).
#pragma once

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace {

// Make `device` the calling thread's, refusing one that is not there.  count_may_fail: a failing hipGetDeviceCount means "none visible"
// instead of an error of its own (lr_psis).
int use_device(int device, const char* who, bool count_may_fail = false) {
    int ndev = 0;
    if (!count_may_fail) LR_HIP(hipGetDeviceCount(&ndev));
    else if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    if (device < 0 || device >= ndev) return fail(LR_ERR_HIP, "%s: device %d not available (%d visible)", who, device, ndev);
    LR_HIP(hipSetDevice(device));
    return LR_OK;
}

// what a result holds before the first draw
void fill_nan(double* v, size_t count) { std::fill(v, v + count, (double)NAN); }

void free_all(std::initializer_list<void*> ptrs) {
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
}

// A grow-only device workspace.  One policy: the old buffer is freed first (hipFree waits for the work that still reads it), then the new
// one is allocated, so a regrow never holds both.  If the allocation fails the workspace is empty and grows again at the next call.
struct Workspace {
    void* p = nullptr;
    size_t bytes = 0;
    int grow(size_t want, const char* who, const char* what) {
        if (bytes >= want) return LR_OK;
        release();
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return fail(LR_ERR_NOMEM, "%s: allocating %zu bytes of %s failed", who, want, what);
        }
        bytes = want;
        return LR_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// Base of an accumulator: what the staging loop keeps between calls.
struct Staged {
    hipStream_t last = nullptr;  // stream of the last accumulate call that got as far as enqueueing: results and resets follow it
    Workspace in, padded;        // host input staged on the device; items padded to the kernel's width
};

// What one accumulate call was given: `count` items at `src` (host memory unless on_device), to be folded in on stream `st`.
struct Feed {
    const void* src;
    int64_t count;
    bool on_device;
    hipStream_t st;
};

// The most one piece stages on the device.  The piece boundaries decide the launch sequence, and with it the bytes of the result.
constexpr size_t kStageBytes = size_t(256) << 20;
// Pieces are kStageBytes / k_item items, at least `least`; device input of a `device_whole` accumulator is one piece whatever its size.
struct Piecing { int64_t least; bool device_whole; };
constexpr Piecing kModelDraws{1024, false};  // draws of a model: device input too (bounds the padded copy and the launch grid)
constexpr Piecing kBlockSteps{1, true};      // time steps of a [k][C][p] block: only host input needs a staging buffer

// The staging loop.  Items of in_item bytes become items of k_item bytes (pad(src, n, dst, st) when the two differ) and go to
// fold(d_items, n, st), which enqueues the launches of one device-resident piece and counts it.  In order:
//   - every workspace is grown for the first piece, which is the largest, and reserve(first) grows the accumulator's own, before anything
//     is enqueued or counted: running out of memory leaves the accumulator as it was;
//   - host input: the stream is synchronised before the staging buffer is overwritten with the next piece, and once at the end, so the
//     caller's memory is free on return.  Device input is only enqueued.
template <typename Pad, typename Reserve, typename Fold>
int stage(const char* who, Staged& s, const Feed& f, size_t in_item, size_t k_item, Piecing pc, Pad&& pad, Reserve&& reserve, Fold&& fold) {
    const bool pads = k_item != in_item;
    const int64_t piece = f.on_device && pc.device_whole ? f.count : std::max<int64_t>(pc.least, (int64_t)(kStageBytes / k_item));
    const int64_t first = std::min(piece, f.count);
    if (!f.on_device)
        if (const int rc = s.in.grow((size_t)first * in_item, who, "staged draws")) return rc;
    if (pads)
        if (const int rc = s.padded.grow((size_t)first * k_item, who, "padded draws")) return rc;
    if (const int rc = reserve(first)) return rc;
    s.last = f.st;
    for (int64_t i0 = 0; i0 < f.count; i0 += piece) {
        const int64_t n = std::min(piece, f.count - i0);
        const void* d = static_cast<const unsigned char*>(f.src) + (size_t)i0 * in_item;
        if (!f.on_device) {
            if (i0) LR_HIP(hipStreamSynchronize(f.st));  // the staging buffer is about to be overwritten
            LR_HIP(hipMemcpyAsync(s.in.p, d, (size_t)n * in_item, hipMemcpyHostToDevice, f.st));
            d = s.in.p;
        }
        if (pads) {
            if (const int rc = pad(d, n, s.padded.p, f.st)) return rc;
            d = s.padded.p;
        }
        if (const int rc = fold(d, n, f.st)) return rc;
    }
    if (!f.on_device) LR_HIP(hipStreamSynchronize(f.st));
    return LR_OK;
}

template <typename T>
int pad_draws(const void* src, int64_t S, int p, int P, void* dst, hipStream_t st) {
    hipLaunchKernelGGL(lr::k_predict_pad<T>, dim3((unsigned)(((size_t)S * P + 255) / 256)), dim3(256), 0, st, static_cast<const T*>(src), S, p, P, static_cast<T*>(dst));
    LR_HIP(hipGetLastError());
    return LR_OK;
}

// draws [S][p] of model m, padded to its kernels' width P where p != P
template <typename Reserve, typename Fold>
int stage_draws(const char* who, Staged& s, const lr_model* m, const Feed& f, Reserve&& reserve, Fold&& fold) {
    const auto pad = [m](const void* src, int64_t n, void* dst, hipStream_t st) { return LR_BY_DTYPE(m->dtype, pad_draws, src, n, m->p, m->P, dst, st); };
    return stage(who, s, f, (size_t)m->p * m->esize(), (size_t)m->P * m->esize(), kModelDraws, pad, reserve, fold);
}

// time steps [k][row bytes] of a block, as they are
template <typename Fold>
int stage_block(const char* who, Staged& s, size_t row, const Feed& f, Fold&& fold) {
    return stage(who, s, f, row, row, kBlockSteps, [](const void*, int64_t, void*, hipStream_t) { return LR_OK; }, [](int64_t) { return LR_OK; }, fold);
}

}  // namespace
