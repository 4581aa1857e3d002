// What the ragged device calls (resample.h, wave_out.h) share: the block lookup and the fixed-tree block sum of their kernels, the tap-table
// staging, and on the host the grow-only device buffers of a per-device workspace.  Each of the two includes it (and rate_pair.h) itself.
#pragma once
#include "rate_pair.h"

constexpr int kLdsMax = 160 * 1024;           // LDS of one CU

// last of the n entries e[] whose member `first` (its first block, sample, ...: ascending over e[]) is at or before b
template <auto first, typename T, typename B>
F5_DEVICE int last_at_or_before(const T* e, int n, B b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (e[mid].*first <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sum of red[0 .. 256) by a fixed binary tree, by a block of 256 threads; every thread returns the total
template <typename T>
F5_DEVICE T block_sum(T* red, int tid, T v) {
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T total = red[0];
    __syncthreads();
    return total;
}

// the tap table (nt floats) into LDS at tp (16-byte aligned) by a block of 256 threads: 16-byte loads where the table's address allows
F5_DEVICE void stage_taps(float* tp, const float* __restrict__ taps, int nt, int tid) {
    if ((reinterpret_cast<uintptr_t>(taps) & 15) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(taps);
        for (int i = tid; i < nt / 4; i += 256) reinterpret_cast<float4*>(tp)[i] = t4[i];
        for (int i = (nt & ~3) + tid; i < nt; i += 256) tp[i] = taps[i];
    } else {
        for (int i = tid; i < nt; i += 256) tp[i] = taps[i];
    }
}

// grows the device buffer *p (capacity *cap elements) to at least `need` elements; its contents are not kept
template <typename T>
static int dev_reserve(T** p, size_t* cap, size_t need, const char* what) {
    if (need <= *cap) return 0;
    dev_free(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, sizeof(T) * need) != hipSuccess) { *p = nullptr; return fail(-5, "hipMalloc %s", what); }
    *cap = need;
    return 0;
}

// the current device's workspace of type W (one per device ordinal, kept for the life of the process), or null with the error set (-6)
template <typename W>
static W* device_workspace(const char* call) {
    static W table[32];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { fail(-6, "%s: hipGetDevice", call); return nullptr; }
    return &table[dev & 31];
}

// A per-device workspace is one set of tables and scratch for every call of its kind, whatever stream the call names.  Its calls take turns:
// WorkspaceTurn turn(ws.use, st) right after device_workspace<W>() makes st wait (on the device, never on the host) for the workspace's
// previous use where that went to another stream, and on every exit of the scope records the end of this use behind what the call queued.
// On one stream a turn is one event record.  The calls themselves arrive one at a time per device from the host (include/f5hip.h).
struct WorkspaceUse { hipEvent_t done = nullptr; hipStream_t last = nullptr; bool recorded = false; };
struct WorkspaceTurn {
    WorkspaceUse& use; hipStream_t st; int rc = 0;
    WorkspaceTurn(WorkspaceUse& u, hipStream_t s) : use(u), st(s) {
        if (!use.done && hipEventCreateWithFlags(&use.done, hipEventDisableTiming) != hipSuccess) { use.done = nullptr; rc = fail(-5, "hipEventCreate workspace turn"); return; }
        if (use.recorded && use.last != st && hipStreamWaitEvent(st, use.done, 0) != hipSuccess) rc = fail(-6, "workspace turn: hipStreamWaitEvent");
    }
    ~WorkspaceTurn() {
        if (!use.done || rc) return;
        if (hipEventRecord(use.done, st) == hipSuccess) { use.recorded = true; use.last = st; }
    }
    WorkspaceTurn(const WorkspaceTurn&) = delete;
    WorkspaceTurn& operator=(const WorkspaceTurn&) = delete;
};
