// cand.h -- the device front end of SampleLogits: what of the logits reaches the host when a token is sampled.
// Host-only plain C++ (no HIP), the idiom of gemv_plan.h: the launch plan, the argument block of cand.hip's launcher,
// a CPU model of the device pass (cand_front_ref) and the tail of ksamp::top_k that starts from the survivors
// (top_k_from_survivors).  tests/test_sample_front.py holds the two to ksamp::top_k without a GPU.
//
// ksamp::top_k for k > 128 buckets every candidate by int(6.4f * logit + 64.f) clamped to [0, 127], walks the buckets
// from 127 down until the running count reaches k (bucket ib), scatters the candidates of buckets >= ib into
// per-bucket runs IN ID ORDER, std::sorts each run above ib and partial_sorts bucket ib.  Everything after the walk
// reads only the survivors in ascending id and the per-bucket counts, so a device pass that returns exactly those
// (plus the 128 totals and ib) lets the host run the same scatter and the same sorts on the same sequences: the
// result is equal entry for entry, the order of equal logits included.  The sorts stay on the host because
// std::sort's order of equal keys is the library's, not a property a device sort could restate.
//
// What touches the logits before top_k(5000) is sparse: set-to-low ids (EOS / EOT suppression, token bans, antislop;
// low = lowest_logit(raw logits), the one scalar that needs every logit), logit biases (f32 +, in list order, ids may
// repeat) and the DRY penalties (f32 -).  The device applies them to a scratch copy; the model's logits stay as they are.
//
// The passes (cand.hip), over n f32 logits in slices of CAND_SLICE consecutive ids, one workgroup each:
//   copy + min   only with edits: scratch = logits, per-slice minimum (ignoring NaN)
//   apply        only with edits: low from the slice minima; one thread per distinct id walks that id's edits in order
//   histogram    128 LDS bins per slice, written out per slice; n_bad = values that are not finite or whose
//                |6.4 v + 64| >= 2^31 (the x86 and GPU float -> int conversions differ there), plus, with a set-low
//                list, raw logits that are not finite (std::min_element's answer then depends on their place)
//   cut          one workgroup: bucket totals, the walk down to ib, per-slice survivor counts scanned into offsets
//   compact      each slice writes its (id, logit) of bucket >= ib at its offset in ascending id, up to cap entries
// The bucket is 6.4f * v + 64.f with both roundings (never an FMA), 0 unless > 0, 127 from 127 up, else truncated: for
// every value the host's int conversion defines, the same bucket as the host's; defined (and equal between the device
// and cand_front_ref) for the others too, which n_bad reports.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sampler.h"

namespace kcand {

constexpr int CAND_NB = 128;             // ksamp::top_k's buckets
constexpr int CAND_K = 5000;             // SampleLogits' pre-filter
constexpr int CAND_CAP = 16384;          // survivors the front end carries; more: the caller falls back
constexpr int CAND_FIRST = 8192;         // entries that come back with the header in one transfer
constexpr int CAND_SLICE = 1024, CAND_BLOCK = 256;
constexpr int CAND_MAX_N = 1 << 22;      // 4096 slices: what the cut's one workgroup scans

struct Edit { int32_t id; float v; };    // (id, bias) or (id, penalty)
struct Hdr {                             // the result header
    float low;                           // lowest_logit(raw logits); 0 without a set-low list (no min pass ran)
    int32_t ib;                          // the cut bucket
    int32_t nhave;                       // survivors = candidates of bucket >= ib (may exceed the capacity)
    int32_t n_bad;                       // > 0: the host's bucket of some value is not defined; fall back
    int32_t hist[CAND_NB];
};
struct HdrM {                            // the masked entries' header: the old one, then the mask's counts
    Hdr h;                               // with ib == 0: nhave = n - n_rej (every non-rejected id comes back)
    int32_t n_rej;                       // ids the mask rejects
    int32_t pad;
};
struct Pair { int32_t id; float v; };    // a survivor as the device writes it
// an edit as the device walks it: sorted by (id, kind), list order kept within a kind
enum { CAND_SET = 0, CAND_ADD = 1, CAND_SUB = 2 };
struct Op { int32_t id, kind; float v; };

struct Plan {
    int rc;                              // 0, or -2: n outside [1, CAND_MAX_N]
    int slice, block, nblk;
};
inline int plan(int64_t n, Plan *p) {
    *p = Plan{};
    p->slice = CAND_SLICE, p->block = CAND_BLOCK;
    if (n < 1 || n > CAND_MAX_N) return p->rc = -2;
    p->nblk = (int)((n + CAND_SLICE - 1) / CAND_SLICE);
    return p->rc = 0;
}

// device workspace of one front end for up to n logits, max_ops edits and cap survivors: byte offsets into one
// allocation (every part 16-byte aligned)
struct WsLayout { size_t scratch, minpart, hist, bad, off, low, ops, out, mask, rej, bytes; };
inline size_t mask_words(int64_t n) { return (size_t)((n + 31) / 32); }
inline WsLayout ws_layout(int64_t n, int64_t max_ops, int64_t cap) {
    Plan p;
    plan(std::max<int64_t>(1, std::min<int64_t>(n, CAND_MAX_N)), &p);
    WsLayout w{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~(size_t)15; return o; };
    w.scratch = take((size_t)n * 4);
    w.minpart = take((size_t)p.nblk * 4);
    w.hist = take((size_t)p.nblk * CAND_NB * 4);
    w.bad = take((size_t)p.nblk * 4);
    w.off = take((size_t)p.nblk * 4);
    w.low = take(4);
    w.ops = take((size_t)max_ops * sizeof(Op));
    w.out = take(sizeof(HdrM) + (size_t)cap * sizeof(Pair));
    w.mask = take(mask_words(n) * 4);
    w.rej = take((size_t)p.nblk * 4);
    w.bytes = at;
    return w;
}

// what cand.hip's launcher takes: device pointers throughout
struct Args {
    const float *logits;
    int n, k, cap;
    const Op *ops;                       // nops edits sorted by (id, kind); n_set > 0: some of them set to low
    int nops, n_set;
    float *scratch, *minpart, *low;
    int32_t *hist, *bad, *off;
    void *out;                           // Hdr, then cap Pairs; with a mask: HdrM, then cap Pairs
    const uint32_t *mask;                // null, or (n + 31) / 32 words: bit i % 32 of word i / 32 set = id i rejected
    int32_t *rej;                        // with a mask: per-slice rejected counts
};

// the edit lists as one sorted program: ops by (id, kind) with the list order kept within a kind, repeated set-low ids
// dropped (setting twice sets once).  keys: scratch the caller may keep.  Returns the number of ops written, -1 when an
// id is outside [0, n), -2 when more than max_ops are needed.
inline int64_t build_ops(int n, const int32_t *set_ids, int n_set, const Edit *adds, int n_add, const Edit *subs, int n_sub,
                         std::vector<uint64_t> &keys, Op *ops, int64_t max_ops) {
    keys.clear();
    auto key = [](int32_t id, int kind, uint32_t seq) { return ((uint64_t)(uint32_t)id << 34) | ((uint64_t)kind << 32) | seq; };
    for (int i = 0; i < n_set; ++i) {
        if (set_ids[i] < 0 || set_ids[i] >= n) return -1;
        keys.push_back(key(set_ids[i], CAND_SET, (uint32_t)i));
    }
    for (int i = 0; i < n_add; ++i) {
        if (adds[i].id < 0 || adds[i].id >= n) return -1;
        keys.push_back(key(adds[i].id, CAND_ADD, (uint32_t)i));
    }
    for (int i = 0; i < n_sub; ++i) {
        if (subs[i].id < 0 || subs[i].id >= n) return -1;
        keys.push_back(key(subs[i].id, CAND_SUB, (uint32_t)i));
    }
    if (!std::is_sorted(keys.begin(), keys.end())) std::sort(keys.begin(), keys.end());     // the keys are distinct
    int64_t no = 0;
    for (const uint64_t kx : keys) {
        const int32_t id = (int32_t)(kx >> 34);
        const int kind = (int)((kx >> 32) & 3);
        const uint32_t seq = (uint32_t)kx;
        if (kind == CAND_SET && no > 0 && ops[no - 1].id == id && ops[no - 1].kind == CAND_SET) continue;
        if (no >= max_ops) return -2;
        ops[no++] = Op{id, kind, kind == CAND_SET ? 0.0f : (kind == CAND_ADD ? adds[seq].v : subs[seq].v)};
    }
    return no;
}

// the device's bucket of an edited value, restated: f = 6.4f * v + 64.f in two roundings (the build keeps the host
// from contracting it, -ffp-contract=off; top_k_from_survivors checks what it got)
inline float bucket_f(float v) {
    volatile float m = 6.4f * v;         // volatile: a product rounded to f32 whatever the contraction setting
    return m + 64.0f;
}
inline int bucket_of(float f) { return !(f > 0.0f) ? 0 : (f >= 127.0f ? 127 : (int)f); }
inline bool value_bad(float v) { return !std::isfinite(v) || !(std::fabs(bucket_f(v)) < 2147483648.0f); }

// the device pass on the CPU: header and the first min(nhave, cap) survivors (id, logit) in ascending id.
// Returns 0, or -1 / -2 as build_ops and plan do.
// mask: null, or the reject bitmask; *n_rej its count over [0, n).
inline int cand_front_ref_masked(const float *logits, int n, int k, const int32_t *set_ids, int n_set, const Edit *adds,
                                 int n_add, const Edit *subs, int n_sub, const uint32_t *mask, Hdr *hdr, int32_t *n_rej,
                                 std::vector<int32_t> &ids, std::vector<float> &vals, int cap) {
    Plan p;
    if (plan(n, &p)) return -2;
    std::vector<uint64_t> keys;
    std::vector<Op> ops((size_t)n_set + n_add + n_sub + 1);
    const int64_t nops = build_ops(n, set_ids, n_set, adds, n_add, subs, n_sub, keys, ops.data(), (int64_t)ops.size());
    if (nops < 0) return (int)nops;
    std::vector<float> e(logits, logits + n);
    float low = 0.0f;
    if (n_set > 0) {
        float m = INFINITY;
        for (int i = 0; i < n; ++i) m = logits[i] < m ? logits[i] : m;
        low = m < 0 ? m - 8 : 0;
    }
    for (int64_t i = 0; i < nops; ++i) {
        float &v = e[ops[i].id];
        if (ops[i].kind == CAND_SET) v = low;
        else if (ops[i].kind == CAND_ADD) v = v + ops[i].v;
        else v = v - ops[i].v;
    }
    *hdr = Hdr{};
    hdr->low = low;
    std::vector<uint8_t> b(n);
    int nrej = 0;
    auto rejected = [&](int i) { return mask && ((mask[i >> 5] >> (i & 31)) & 1u); };
    for (int i = 0; i < n; ++i) {
        b[i] = rejected(i) ? 0 : (uint8_t)bucket_of(bucket_f(e[i]));
        nrej += rejected(i);
        ++hdr->hist[b[i]];
        if (value_bad(e[i]) || (n_set > 0 && !std::isfinite(logits[i]))) ++hdr->n_bad;
    }
    k = std::min(std::max(k, 1), n);
    int nhave = 0, ib = CAND_NB - 1;
    for (; ib >= 0; --ib) {
        nhave += hdr->hist[ib];
        if (nhave >= k) break;
    }
    if (mask && ib == 0) nhave = n - nrej;
    hdr->ib = ib, hdr->nhave = nhave;
    if (n_rej) *n_rej = nrej;
    ids.clear(), vals.clear();
    for (int i = 0; i < n && (int)ids.size() < cap; ++i)
        if (b[i] >= ib && !rejected(i)) { ids.push_back(i); vals.push_back(e[i]); }
    return 0;
}
inline int cand_front_ref(const float *logits, int n, int k, const int32_t *set_ids, int n_set, const Edit *adds, int n_add,
                          const Edit *subs, int n_sub, Hdr *hdr, std::vector<int32_t> &ids, std::vector<float> &vals, int cap) {
    return cand_front_ref_masked(logits, n, k, set_ids, n_set, adds, n_add, subs, n_sub, nullptr, hdr, nullptr, ids, vals, cap);
}

// The cut in bucket 0 under a mask: the n-entry candidate array the full chain would have had after sample_grammar --
// rejected ids -inf, every other id its edited value from the front end -- ready for ksamp::top_k(k).  false: the
// survivors are not exactly the non-rejected ids in ascending order (the caller runs the full chain).
inline bool rebuild_masked(const Hdr &hdr, int n_rej, const uint32_t *mask, const int32_t *ids, const float *vals, int nsurv,
                           int n, std::vector<ksamp::TokData> &out) {
    if (hdr.ib != 0 || nsurv != hdr.nhave || nsurv != n - n_rej) return false;
    out.resize(n);
    int at = 0;
    for (int i = 0; i < n; ++i) {
        if ((mask[i >> 5] >> (i & 31)) & 1u) { out[i] = ksamp::TokData{i, -INFINITY, 0.0f}; continue; }
        if (at >= nsurv || ids[at] != i) return false;
        out[i] = ksamp::TokData{i, vals[at++], 0.0f};
    }
    return at == nsurv;
}

// The tail of ksamp::top_k(c, k) for k > 128 from a front-end result: scatter into per-bucket runs, the sorts, take k.
// Each survivor's bucket is derived again with top_k's own expression; a survivor below the cut, per-bucket counts
// other than the header's, a header whose totals are not n or whose cut is not the walk's: false ("mismatch", the
// caller runs the full chain) -- the guard against a host build that rounds the bucket expression differently.
// nsurv = hdr.nhave (the caller has checked the capacity and n_bad).  out: the k candidates, p = 0, as top_k leaves them.
inline bool top_k_from_survivors(const Hdr &hdr, const int32_t *ids, const float *vals, int nsurv, int n, int k,
                                 std::vector<ksamp::TokData> &out) {
    using ksamp::TokData;
    constexpr int nb = CAND_NB;
    constexpr float lo = -10.0f, hi = 10.0f;
    constexpr float scale = nb / (hi - lo);
    constexpr float inter = -lo * scale;
    const int ib = hdr.ib;
    k = std::min(std::max(k, 1), n);
    if (k <= 128 || ib < 0 || ib >= nb || nsurv != hdr.nhave) return false;
    int64_t total = 0, nhave = 0;
    for (int j = 0; j < nb; ++j) {
        if (hdr.hist[j] < 0) return false;
        total += hdr.hist[j];
        if (j >= ib) nhave += hdr.hist[j];
    }
    if (total != n || nhave != nsurv || nhave < k || nhave - hdr.hist[ib] >= k) return false;
    auto comp = [](const TokData &a, const TokData &b) { return a.logit > b.logit; };
    std::vector<TokData> tmp(nsurv);
    TokData *ptr = tmp.data();
    std::vector<TokData *> bptr;
    bptr.reserve(nb - ib);
    for (int j = nb - 1; j >= ib; --j) { bptr.push_back(ptr); ptr += hdr.hist[j]; }
    int cnt[nb] = {0};
    for (int i = 0; i < nsurv; ++i) {
        if (ids[i] < 0 || ids[i] >= n || (i > 0 && ids[i] <= ids[i - 1])) return false;
        int j = int(scale * vals[i] + inter);
        j = std::max(0, std::min(nb - 1, j));
        if (j < ib || ++cnt[j] > hdr.hist[j]) return false;
        *bptr[nb - 1 - j]++ = TokData{ids[i], vals[i], 0.0f};
    }
    for (int j = ib; j < nb; ++j)
        if (cnt[j] != hdr.hist[j]) return false;
    ptr = tmp.data();
    int ndone = 0;
    for (int j = nb - 1; j > ib; --j) {
        std::sort(ptr, ptr + hdr.hist[j], comp);
        ptr += hdr.hist[j];
        ndone += hdr.hist[j];
    }
    std::partial_sort(ptr, ptr + k - ndone, ptr + hdr.hist[ib], comp);
    out.assign(tmp.begin(), tmp.begin() + k);
    return true;
}

}  // namespace kcand

// cand.hip: enqueue the passes on the stream; 0, or a negative code (-2 bad arguments, -1 launch failure)
int kcpp_cand_launch(const kcand::Plan &p, const kcand::Args &a, void *stream);
