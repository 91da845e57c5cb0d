// Host-side planning of the loss-term table (csrc/depth_gt.hip): argument checks that need no device, the integer ratios of a
// ground-truth term and the block prefix that deals the workgroups of ONE launch to the terms.  Plain C++ without HIP, so that
// scripts/dev/loss_plan_check.cpp compiles it stand-alone under the host sanitizers.
#pragma once

namespace pscv {

constexpr int LOSS_MAX_TERMS = 32;          // = PSCV_LOSS_MAX_TERMS (static_assert in depth_gt.hip)
constexpr int LOSS_BLOCK = 256;             // threads of a reduce / backward workgroup
constexpr int LOSS_PER_THREAD = 4;          // consecutive pixels per thread and step (one 16-byte load where alignment allows)
constexpr int LOSS_CHUNK = LOSS_BLOCK * LOSS_PER_THREAD;
constexpr int LOSS_MAX_BLOCKS_PER_TERM = 256;   // a term with more chunks walks them with this stride; the finish reads <= 256 partials per term

struct LossPlan {
    int n_terms;
    int blk_start[LOSS_MAX_TERMS + 1];      // term t owns workgroups [blk_start[t], blk_start[t + 1])
    int rh[LOSS_MAX_TERMS], rw[LOSS_MAX_TERMS];   // H / h, W / w of the ground-truth kinds; 1 for the others
    long npix[LOSS_MAX_TERMS];              // b h w
    const char* error;                      // static text of the first problem (null = none) and the term it was found at
    int error_term;
};

inline bool loss_kind_has_gt(int kind) { return kind == 0 || kind == 1; }
inline bool loss_kind_has_u(int kind) { return kind == 1 || kind == 3; }

// kinds [n], dims [n][5] = (b, h, w, H, W).  Returns false with plan.error set on the first bad argument; never reads past n
// entries, never writes outside `plan`.
inline bool loss_plan(int n_terms, const int* kinds, const long* dims, LossPlan& plan) {
    plan.n_terms = 0;
    plan.error = nullptr;
    plan.error_term = -1;
    plan.blk_start[0] = 0;
    auto fail = [&](const char* msg, int t) { plan.error = msg; plan.error_term = t; return false; };
    if (!kinds || !dims) return fail("null pointer argument (kinds / dims)", -1);
    if (n_terms < 1) return fail("no terms", -1);
    if (n_terms > LOSS_MAX_TERMS) return fail("more than 32 terms in one call", -1);
    for (int t = 0; t < n_terms; ++t) {
        const long* d = dims + 5L * t;
        const int kind = kinds[t];
        if (kind < 0 || kind > 3) return fail("unknown kind", t);
        if (d[0] <= 0 || d[1] <= 0 || d[2] <= 0) return fail("zero or negative size", t);
        // b h w < 2^31 without overflowing on the way
        const long lim = 0x7fffffffL;
        if (d[0] > lim || d[1] > lim || d[2] > lim || d[1] * d[2] > lim || d[0] * (d[1] * d[2]) > lim)
            return fail("more than 2^31 - 1 pixels in one term", t);
        plan.npix[t] = d[0] * d[1] * d[2];
        plan.rh[t] = plan.rw[t] = 1;
        if (loss_kind_has_gt(kind)) {
            if (d[3] <= 0 || d[4] <= 0) return fail("zero or negative ground-truth size", t);
            if (d[3] > lim || d[4] > lim || d[3] * d[4] > lim) return fail("ground truth larger than 2^31 - 1 pixels per image", t);
            if (d[3] % d[1] || d[4] % d[2]) return fail("non-integer ratio between the ground truth and the depth map", t);
            plan.rh[t] = (int)(d[3] / d[1]);
            plan.rw[t] = (int)(d[4] / d[2]);
        }
        long nb = (plan.npix[t] + LOSS_CHUNK - 1) / LOSS_CHUNK;
        if (nb > LOSS_MAX_BLOCKS_PER_TERM) nb = LOSS_MAX_BLOCKS_PER_TERM;
        plan.blk_start[t + 1] = plan.blk_start[t] + (int)nb;        // <= 32 * 256
    }
    plan.n_terms = n_terms;
    return true;
}

}  // namespace pscv
