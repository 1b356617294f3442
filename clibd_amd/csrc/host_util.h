// Host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace clibd {

// thread-local last-error text (defined in capi.hip)
char* last_error_buf();
constexpr int kErrBufLen = 256;

inline int set_error(int code, const char* msg) {
    snprintf(last_error_buf(), kErrBufLen, "%s", msg);
    return code;
}

// "op: what" as the last error; returns CLIBD_EINVAL (-1): the argument checks that serve several entry points name the one that was called
inline int fail(const char* op, const char* what) {
    snprintf(last_error_buf(), kErrBufLen, "%s: %s", op, what);
    return -1;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int pad64(int v) { return (v + 63) / 64 * 64; }
inline int pad16(int v) { return (v + 15) / 16 * 16; }

// Carves a caller-owned workspace into pieces, each rounded up to 256 bytes.  A null base yields null pointers: the size queries run the
// same carve function as their entry point and return total().
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    template <typename T>
    T* take(size_t count) {
        char* p = base ? base + off : nullptr;
        off += align_up(count * sizeof(T), 256);
        return (T*)p;
    }
    size_t total() const { return off; }
};

// The workspace rule of the reduction entry points (include/clibd_hip.h, "deterministic mode"): NULL with size 0 selects the atomic / plain
// form; NULL with a size, a misaligned or a short workspace is CLIBD_EINVAL, and the message names the size query.  `need` = that query's answer.
inline int check_workspace(const char* op, const char* name, const void* ws, size_t bytes, size_t need, const char* query) {
    if (ws == nullptr ? bytes == 0 : (aligned16(ws) && bytes >= need)) return 0;
    char msg[kErrBufLen];
    if (ws == nullptr) snprintf(msg, sizeof msg, "%s: %s size without a %s", op, name, name);
    else snprintf(msg, sizeof msg, "%s: %s too small or misaligned (%s)", op, name, query);
    return set_error(-1, msg);
}

// Launch-time errors only (no synchronisation): configuration errors surface here, device faults do not.
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(last_error_buf(), kErrBufLen, "%s: %s", what, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

// grid size for a grid-stride elementwise kernel: ceil(n / per_block), capped
inline unsigned grid_for(size_t n, int per_block = 256, unsigned cap = 4096) {
    size_t b = (n + per_block - 1) / per_block;
    if (b > cap) b = cap;
    return b < 1 ? 1u : (unsigned)b;
}

// out[c] += sum_b partials[b * C + c] (c < split; out_b[c - split] for the rest) in an order that depends on (nblk, C) only:
// the fixed-order second kernel of every partials-workspace form (gemm.hip).  Returns check_launch's code.
int ordered_colsum_launch(const float* partials, int nblk, int C, float* out, int split, float* out_b, hipStream_t stream);

}  // namespace clibd
