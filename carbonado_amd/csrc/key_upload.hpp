// key_upload.hpp — how a table that holds keys reaches the device
// (api_ecies.cpp, api_cread.cpp): through a pinned copy that a host function
// enqueued behind the upload wipes, the pageable table wiped before the call
// returns.
#pragma once

#include "api_common.hpp"

namespace chip {
namespace api {

// The pinned copy of a call's table (it holds the keys).  One per thread: the
// next call waits for the previous upload and wipe before it refills it.
struct KeyStage {
    DevBuf pin;
    hipEvent_t ev = nullptr;
    bool armed = false;
};
inline thread_local KeyStage t_key_stage;

// what the host function behind an upload wipes (its own allocation, so that
// it outlives the thread that made the call)
struct KeyWipe {
    void *p;
    size_t n;
};

inline void key_wipe_cb(void *u) {
    auto *w = static_cast<KeyWipe *>(u);
    host::secure_wipe(w->p, w->n);
    delete w;
}

inline hipError_t upload_key_table(std::vector<uint8_t> &table, void *dst, hipStream_t s) {
    KeyStage &k = t_key_stage;
    hipError_t e = hipSuccess;
    if (k.armed) {
        e = hipEventSynchronize(k.ev);
        k.armed = false;
    }
    if (e == hipSuccess && !k.ev) e = hipEventCreateWithFlags(&k.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = grow_pinned(k.pin, table.size());
    if (e != hipSuccess) {
        host::secure_wipe(table.data(), table.size());
        return e;
    }
    const size_t n = table.size();
    std::memcpy(k.pin.p, table.data(), n);
    host::secure_wipe(table.data(), n);
    e = hipMemcpyAsync(dst, k.pin.p, n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        host::secure_wipe(k.pin.p, n);
        return e;
    }
    KeyWipe *w = new KeyWipe{k.pin.p, n};
    e = hipLaunchHostFunc(s, key_wipe_cb, w);
    if (e != hipSuccess) delete w;  // (the next call overwrites the pinned copy; nothing wipes it before)
    if (e == hipSuccess) e = hipEventRecord(k.ev, s);
    k.armed = true;
    return e;
}

}  // namespace api
}  // namespace chip
