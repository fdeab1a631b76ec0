// gemv_plan.h -- which kernel runs a fused single-token mat-vec, with which template instance, grid and LDS.  Host-only
// plain C++ (no HIP), the idiom of gemm_plan.h and fa_plan.h.  The entries (kcpp_gemv_dec, kcpp_gemv_rs, kcpp_gemv_rs_aux,
// kcpp_gemv_q4k, kcpp_gemv_stream, kcpp_gemv_rs_qkv_mixed, kcpp_gemv_qkv_dual) are: gemv_shape_of (kcpp_internal.h, the
// one place that looks at pointers), a plan from here, the kernel file's launcher.  kcpp_gemv_dec_plan exposes the plan,
// tests/test_gemv_plan.py holds it to an independent restatement without a GPU.
//
// The rules, in the order they apply.  rows = N[0] + .. + N[nseg - 1]; nsb = K / 256; "ex" = a q|k|v bias or NeoX pairs.
// Figures are MI355X microseconds per launch; where no tool is named the sweep that gave them is not in the tree.
//
// kcpp_gemv_dec (GEMV_ENTRY_DEC)
//   1. KT_Q4_K_RS / KT_Q5_K_RS / KT_Q6_K_RS: the RS rules below (only the RS kernels read the row-major layouts).
//   2. mode 2 with ex: -3 (the RS kernels only; the caller runs the projection unfused).
//   3. KT_Q4_K: the GEMV_Q4K rules; their answer stands unless it is -3.
//   4. the 17 block types of gemv_unit_type: the GEMV_UNIT rules.  Any other type: -3.
//   GEMV_STREAM is never chosen here: the one shape it covers is GEMV_Q4K's first.  kcpp_gemv_stream runs it.
//
// GEMV_RS (gemv_rs.hip k_gemv_rs; kcpp_gemv_rs restricts the plan to it)
//   gemv_rs_supported(type, K), else -3: K a multiple of 256; activation slices in registers up to 56 (Q4_K, Q5_K) /
//   64 (Q6_K, nsb % 8 == 0) super-blocks, read from LDS (XL) up to the register budget of a row: 112 (Q4_K: K 28672,
//   Llama-3-70B's n_ff), 80 (Q5_K: 12 VGPRs per piece spill past 10 pieces), 128 (Q6_K).
//   NI = ceil(nsb PIECES / 64) pieces per lane per row (PIECES 8, Q6_K 4), MC = ceil(K / 4096) prologue chunks.  Past
//   NI 7 (Q6_K: 4) the XL instances, NI the ceiling the shape rounds up to -- Q6_K 6 / 8, Q5_K 10, Q4_K 10 / 12 / 14 --
//   and MC that ceiling's (NI, Q4_K / Q5_K NI / 2).
//   mode 3 (both MoE top-2 slots' down projections, the Mixtral class): pro 2, one segment, eid, eid1 and escale set,
//     K 14336, else -3.  R 1, 8 waves (4 per slot), cap 256; group prefetch measured no faster (23.2 / 21.7 vs 23.2 /
//     21.0 us) for more registers, so the instance is built without (gemv_rs.hip Q_PF, Q_XL: its compile-time probes).
//   nseg outside 1..3: -3.  mode 1 takes one segment, or two with eid1 or a router (the two MoE slots), else -3.
//   mode 2 with ex: dense weights (no eid, no router), roles in 0..2, with NeoX whole heads of even D >= 2 in the q / k
//     segments, pro 1, no aux and not XL, else -3.  The EX instance: R 2, 4 waves, cap 512.
//   XL: no aux.  mode 0: pro 0 / 1 / 2 (pro 0: the M <= 8 prefill tail and the plugin's few-row MUL_MAT, gemv_cols);
//     mode 1: pro 0 / 1, no router, one segment or eid1; mode 2: pro 1, R 2.  Else -3.  R 1, 8 waves, cap 256, no
//     prefetch: a row's NI pieces are already 16 KB (Q4_K, K 28672) in flight per wave, 128 KB per CU.
//   Otherwise R, PF and the grid cap by shape:
//     gate|up (mode 1)        R 1, PF, 512          14.8 us / 66 MB
//     q|k|v (mode 2)          R 2, 512               7.0 us / 14 MB
//     head (rows > 16384)     R 2, 512              69.4 us / 431 MB (6.2 TB/s)
//     down (K > 8192)         R 1, PF (Q4_K only), 256 (Q4_K) / 512      12.5 / 15.0 us
//     wo (pro 2, 4 waves)     R 1, 512              (1024: every workgroup quantizes the input, more of them cost more;
//                                                    since the 8-wave form below only a mode outside 0..3 gets here)
//     other                   R 1, 1024              4.9 us / 9.4 MB
//   and 8-wave workgroups at cap 256 (one activation prologue shared by 8 waves instead of 4) for the GLU with the
//   norm prologue (mode 1, pro 1, PF) and for mode 0 with pro 2 up to 16384 rows.  Per kernel in isolation
//   (tools/stream_probe.py dec, weights rotated past the Infinity Cache): GLU 14.8 -> 14.1, down Q4_K 11.3 -> 9.7 and
//   Q6_K 13.6 -> 12.2 (no PF: two rows per wave, both in flight), wo 5.4 -> 4.7; in the bench's token graph down 12.0 /
//   13.7 -> 10.0 / 12.4, wo 5.3 -> 5.1, GLU unchanged: 577 -> 600 tok/s.  q|k|v stays at 4 waves (8: 6.8 -> 7.4 us,
//   592 tok/s).  A router on that GLU (ROUTE): two segments, 2..8 experts, K <= 4096, F32 / F16 router weight, ids and
//   weights outputs given, else -3.  Any pro outside 0..3: -3.  A mode outside 0..3 runs the table as mode 0.
//   pro 3 (LayerNorm prologue, the Command-R class): dense weights (no eid, eid1, escale, router), no ex, no aux, not XL,
//     and one of: mode 2 (R 2, 4 waves, cap 512); mode 1 with one segment (R 1, PF, 8 waves, cap 256); mode 0 with one
//     segment of more than 16384 rows, the head (R 2, 4 waves, cap 512) -- pro 1's plans of the same shapes.  Else -3,
//     and -3 from every other family (GEMV_Q4K, GEMV_STREAM, GEMV_UNIT) and the mixed launch with ex.
//   A segment whose rows are no multiple of R: -5.
// GEMV_RS_AUX (k_gemv_rs_aux, the ggml plugin's fused nodes; kcpp_gemv_rs_aux)
//   An AuxOut; mode 0 with p0, h0 or a rope, or mode 1 with the GLU triple; a rope only in mode 0, with positions and an
//   even D >= 2; else -3.  pro 1 when DecArgs.nw is set (the norm in the prologue: K <= 4096, one chunk per thread, so
//   the sum order is the plugin's norm kernels'), else pro 2.  Then GEMV_RS's checks, and not XL.
//     rope: mode 0, an even row count <= 16384; R 2 (a rope pair in one lane, as the runtime's q|k|v), 4 waves, cap 512;
//       pro 1 only at MC 1
//     mode 0, pro 2, rows <= 16384: R 1, 8 waves, cap 256
//     mode 1, one segment, no eid, no router: pro 2: R 1, PF, 4 waves, cap 512; pro 1 at MC 1: R 1, PF, 8 waves, cap 256
//     else -3
// GEMV_Q4K (gemv_q4k.hip; kcpp_gemv_q4k): KT_Q4_K, nseg 1..3, not mode 2 with ex, else -3
//     K 4096: (mode 1, pro 1) R 2, PF: 17.5 us vs 21.1 for GEMV_UNIT;  (2, 1) R 2;  (0, 0) R 1;  (0, 1) R 2, PF
//     K 14336, mode 0: pro 2 and pro 0, R 1, no PF (R 2 / prefetch variants no faster)
//     else -3.  A segment whose rows are no multiple of R: -5.
//   Grid cap 512 (2 per CU), 256 for gate|up with R 2: fewer prologues (each workgroup re-derives the activation) and
//   less queueing than 1024 (tools/stream_probe.py sweep).
// GEMV_STREAM (gemv_stream.hip; kcpp_gemv_stream): KT_Q4_K, K % 256 == 0, nseg 1..3, no eid, not mode 2 with ex, and
//   K 14336, mode 0, pro 2 (one row per wave: 20.3 us vs 24.6 for GEMV_UNIT; at K 4096 it loses on VALU work per byte,
//   tools/stream_probe.py); else -3.  Grid cap 1024.
// GEMV_UNIT (gemv_dec_impl.h k_gemv_dec, one translation unit per type)
//   mode 2: pro 1 (else -7), R 2.  mode 1: pro 1 (else -7), R 2 when rows_per_wave >= 2 else 1.  Any other mode runs as
//   mode 0: pro 0: R 4 / 2 / 1 by rows_per_wave >= 4 / >= 2; pro 1: R 2 / 1; any other pro is pro 2, R 1.
//   MC: pro 0: 1; pro 1: 1 or 2 by ceil(K / 4096) <= 1; pro 2: 2 / 4 / 8 by ceil(K / 4096) <= 2 / <= 4.
//   IT = the K slices per lane, ceil(K / ELEMS / 64) rounded up to 1 / 2 / 4 (pro 2: 2 / 4 / 8); past that -8.
//   A segment whose rows are no multiple of R: -5.  A prologue with K > 4096 MC: -6.
//   Grid cap 1024 for K <= 4096 (the output head prefers more), 512 past it (ffn_down's quantize prologue: 20.6 vs
//   26.8 us).  No result slots, so no floor.
//
// Grids.  The kernels with per-lane result slots (RS, Q4K, STREAM) launch min(ceil(groups / WPG), cap) workgroups and
// at least ceil(groups / (SLOTS WPG)): groups = rows / R, WPG = waves per workgroup (mode 3: half of them), SLOTS = 64
// groups per wave (STREAM: LPR tiles).  LDS is the Q8_K activation image K + K / 256 4 + K / 16 2 (+ 16); twice its
// 16-byte round-up in mode 3; STREAM adds its per-wave header tables; UNIT takes its type's activation image.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/kcpp_synth.h"

enum { GEMV_RS = 0, GEMV_RS_AUX = 1, GEMV_Q4K = 2, GEMV_STREAM = 3, GEMV_UNIT = 4 };
// which entry asks: kcpp_gemv_dec, or one family's own entry (the plan restricted to that kernel)
enum { GEMV_ENTRY_DEC = 0, GEMV_ENTRY_RS = 1, GEMV_ENTRY_RS_AUX = 2, GEMV_ENTRY_Q4K = 3, GEMV_ENTRY_STREAM = 4,
       GEMV_ENTRY_UNIT = 5 };
// what of a DecArgs / AuxOut is present (gemv_shape_of)
enum {
    GEMV_F_EID = 1, GEMV_F_EID1 = 2, GEMV_F_ESCALE = 4,
    GEMV_F_ROUTE_W = 8,          // a router weight (its type and expert count: route_wt, route_ne)
    GEMV_F_ROUTE_OUT = 16,       // route_ids and route_wts both given
    GEMV_F_EX = 32,              // a bias or NeoX pairs (dec_args_ex)
    GEMV_F_NEOX = 64,
    GEMV_F_NW = 128,             // DecArgs.nw: the aux entry's norm-in prologue
    GEMV_F_AUX = 256,            // an AuxOut
    GEMV_F_AUX_P0H0 = 512,       // p0 or h0 (so the GLU triple sets it too)
    GEMV_F_AUX_GLU = 1024,       // p0, p1 and p2
    GEMV_F_AUX_ROPE = 2048,      // rope.out
    GEMV_F_AUX_ROPE_OK = 4096,   // rope.pos set and rope.D even, >= 2
};
#define GEMV_ERR_NO_INSTANCE (-30)     // a launcher met a plan that names no built instance: a bug in this file

struct GemvShape {
    int type;
    int64_t K;
    int nseg;
    int64_t N[3];
    int role[3];
    int D;
    int mode, pro, rows_per_wave;
    int flags;                   // GEMV_F_*
    int route_wt, route_ne;
};

struct GemvPlan {
    int rc;                      // 0, or the entry's return code: nothing is launched
    int kernel;                  // GEMV_*
    int type, mode, pro;         // the instance's TYPE, MODE, PRO
    int NI;                      // RS: pieces per lane per row (XL: the ceiling); STREAM: chunks per lane
    int IT;                      // Q4K, UNIT: K slices per lane
    int LPR;                     // STREAM: lanes per row
    int R, MC, PF, waves, XL, ROUTE, EX;
    int64_t nblk;
    int block;
    int64_t lds_bytes;
};

inline int gemv_rows_per_wave(int64_t N, int mode) {
    if (mode == 1) return 1;
    return N > 16384 ? 4 : (N > 4096 ? 2 : 1);
}

inline bool gemv_rs_type(int type) { return type == KT_Q4_K_RS || type == KT_Q5_K_RS || type == KT_Q6_K_RS; }
inline bool gemv_rs_supported(int type, int64_t K) {
    if (K % 256 || K < 256) return false;
    const int64_t nsb = K / 256;
    if (type == KT_Q4_K_RS || type == KT_Q4_K) return nsb <= 112;
    if (type == KT_Q5_K_RS || type == KT_Q5_K) return nsb <= 80;
    if (type == KT_Q6_K_RS || type == KT_Q6_K) return nsb % 8 == 0 && nsb <= 128;
    return false;
}
// unit-per-lane kernels exist for these; ELEMS = elements per unit
inline int gemv_unit_elems(int type) {
    switch (type) {
    case KT_Q4_0: case KT_Q5_0: case KT_Q8_0: case KT_IQ4_NL: return 32;
    case KT_Q4_K: case KT_Q5_K: case KT_Q6_K: case KT_Q3_K: case KT_Q2_K: case KT_IQ4_XS: case KT_IQ2_XXS: case KT_IQ2_XS:
    case KT_IQ2_S: case KT_IQ3_XXS: case KT_IQ3_S: case KT_IQ1_S: case KT_IQ1_M: return 64;
    default: return 0;
    }
}
inline bool gemv_unit_type(int type) { return gemv_unit_elems(type) != 0; }

inline int64_t gemv_rows(const GemvShape &s) {
    int64_t n = 0;
    for (int i = 0; i < s.nseg && i < 3; ++i) n += s.N[i];
    return n;
}
inline bool gemv_rows_split(const GemvShape &s, int R) {     // every segment a whole number of R-row groups
    for (int i = 0; i < s.nseg && i < 3; ++i)
        if (s.N[i] % R) return false;
    return true;
}
inline int64_t gemv_q8k_bytes(int64_t K) { return K + K / 256 * 4 + K / 16 * 2; }
inline int64_t gemv_slot_grid(int64_t groups, int wpg, int cap, int slots) {
    const int64_t nblk = std::min<int64_t>((groups + wpg - 1) / wpg, cap);
    return std::max<int64_t>(nblk, (groups + (int64_t)slots * wpg - 1) / ((int64_t)slots * wpg));
}

// ---- one grid and LDS rule per kernel (p's instance parameters are set)
inline void gemv_rs_grid(int64_t rows, int64_t K, int cap, GemvPlan *p) {
    const int wpg = p->mode == 3 ? p->waves / 2 : p->waves;
    const int64_t ab = gemv_q8k_bytes(K);
    p->nblk = gemv_slot_grid(rows / p->R, wpg, cap, 64);
    p->block = 64 * p->waves;
    p->lds_bytes = (p->mode == 3 ? 2 * ((ab + 15) & ~(int64_t)15) : ab) + 16;
}
inline void gemv_q4k_grid(int64_t rows, int64_t K, GemvPlan *p) {
    p->nblk = gemv_slot_grid(rows / p->R, 4, p->mode == 1 && p->R == 2 ? 256 : 512, 64);
    p->block = 256;
    p->lds_bytes = gemv_q8k_bytes(K) + 16;
}
inline void gemv_stream_grid(int64_t rows, int64_t K, GemvPlan *p) {
    const int G = 64 / p->LPR;
    p->nblk = gemv_slot_grid(rows / G, 4, 1024, p->LPR);
    p->block = 256;
    p->lds_bytes = ((gemv_q8k_bytes(K) + 15) & ~(int64_t)15) + (int64_t)4 * (p->mode == 1 ? 2 : 1) * G * (K / 256) * (16 + 4);
}
inline void gemv_unit_grid(int64_t rows, int64_t K, GemvPlan *p) {
    const bool q80 = gemv_unit_elems(p->type) == 32;         // vec_dot_type: Q8_0 (d f32, sums i16 per 32), else Q8_K
    p->nblk = std::min<int64_t>((rows / p->R + 3) / 4, K > 4096 ? 512 : 1024);
    p->block = 256;
    p->lds_bytes = p->pro ? (q80 ? K + K / 32 * 4 + K / 32 * 2 : gemv_q8k_bytes(K)) + 16 : 0;
}

// ---- the families
// NI, MC, XL of (type, K); false: no instance
inline bool gemv_rs_class(int type, int64_t K, GemvPlan *p) {
    const int q6 = type == KT_Q6_K_RS;
    const int ni = (int)((K / 256 * (q6 ? 4 : 8) + 63) / 64);
    p->XL = ni > (q6 ? 4 : 7);
    if (!p->XL) {
        p->NI = ni;
        p->MC = (int)((K + 4095) / 4096);
        return true;
    }
    if (q6) p->NI = ni <= 6 ? 6 : 8;
    else if (type == KT_Q5_K_RS) p->NI = 10;
    else p->NI = ni <= 10 ? 10 : (ni <= 12 ? 12 : 14);
    p->MC = q6 ? p->NI : p->NI / 2;
    return ni <= p->NI;
}

inline int gemv_rs_plan(const GemvShape &s, bool aux_entry, GemvPlan *p) {
    const int f = s.flags, mode = s.mode;
    const bool ex = f & (GEMV_F_EX | GEMV_F_NEOX), route = f & GEMV_F_ROUTE_W, rope = f & GEMV_F_AUX_ROPE;
    int pro = s.pro;
    p->kernel = aux_entry ? GEMV_RS_AUX : GEMV_RS;
    p->type = s.type;
    if (aux_entry) {
        if (!(f & GEMV_F_AUX) || (mode != 0 && mode != 1)) return -3;
        if (mode == 0 && !(f & (GEMV_F_AUX_P0H0 | GEMV_F_AUX_ROPE))) return -3;
        if (mode == 1 && !(f & GEMV_F_AUX_GLU)) return -3;
        if (rope && (mode != 0 || !(f & GEMV_F_AUX_ROPE_OK))) return -3;
        pro = f & GEMV_F_NW ? 1 : 2;
        if (pro == 1 && (s.K > 4096 || s.K % 256)) return -3;
    }
    if (!gemv_rs_type(s.type) || !gemv_rs_supported(s.type, s.K)) return -3;
    const int64_t rows = gemv_rows(s);
    int cap = 1024;
    p->R = 1, p->PF = 0, p->waves = 4, p->ROUTE = 0, p->EX = 0;
    p->mode = mode == 1 || mode == 2 || mode == 3 ? mode : 0;
    p->pro = pro;
    if (mode == 3) {
        if (pro != 2 || s.nseg != 1 || !(f & GEMV_F_EID) || !(f & GEMV_F_EID1) || !(f & GEMV_F_ESCALE) || s.K != 14336) return -3;
        gemv_rs_class(s.type, s.K, p);
        p->waves = 8, cap = 256;
    } else {
        if (s.nseg < 1 || s.nseg > 3) return -3;
        if (mode == 1 && s.nseg != 1 && !(s.nseg == 2 && ((f & GEMV_F_EID1) || route))) return -3;
        if (mode == 2 && ex) {
            if ((f & GEMV_F_EID) || route) return -3;
            for (int i = 0; i < s.nseg; ++i) {
                if (s.role[i] < 0 || s.role[i] > 2) return -3;
                if ((f & GEMV_F_NEOX) && s.role[i] != 2 && (s.D < 2 || s.D % 2 || s.N[i] % s.D)) return -3;
            }
        }
        if (!gemv_rs_class(s.type, s.K, p)) return -3;
        if (pro == 3) {
            if (aux_entry || p->XL || ex || route || (f & (GEMV_F_EID | GEMV_F_EID1 | GEMV_F_ESCALE))) return -3;
            if (!(mode == 2 || (mode == 1 && s.nseg == 1) || (mode == 0 && s.nseg == 1 && rows > 16384))) return -3;
        }
        if (p->XL) {
            if (aux_entry || (mode == 2 && ex)) return -3;
            if (mode == 0 ? pro < 0 || pro > 2 : (mode == 1 ? pro != 0 && pro != 1 : (mode == 2 ? pro != 1 : true))) return -3;
            if (mode == 1 && (route || (s.nseg != 1 && !(f & GEMV_F_EID1)))) return -3;
            p->R = mode == 2 ? 2 : 1, p->waves = 8, cap = 256;
        } else {
            const bool q4 = s.type == KT_Q4_K_RS;
            if (mode == 1) p->PF = 1, cap = 512;
            else if (mode == 2) p->R = 2, cap = 512;
            else if (rows > 16384) p->R = 2, cap = 512;
            else if (s.K > 8192) p->PF = q4, cap = q4 ? 256 : 512;
            else if (pro == 2) cap = 512;
            if (mode == 2 && ex) {
                if (aux_entry || pro != 1) return -3;
                p->EX = 1;
            } else if (aux_entry) {
                if (rope) {
                    if (rows > 16384 || rows % 2 || (pro == 1 && p->MC != 1)) return -3;
                    p->R = 2, p->PF = 0, cap = 512;
                } else if (mode == 0 && pro == 2 && rows <= 16384) {
                    p->PF = 0, p->waves = 8, cap = 256;
                } else if (mode == 1 && s.nseg == 1 && !(f & GEMV_F_EID) && !route && (pro == 2 || p->MC == 1)) {
                    if (pro == 1) p->waves = 8, cap = 256;
                    else cap = 512;
                } else {
                    return -3;
                }
            } else if (mode == 1 && (pro == 1 || pro == 3)) {
                if (route) {
                    if (p->MC != 1 || s.nseg != 2 || s.route_ne < 2 || s.route_ne > 8 || s.K > 4096 || !(f & GEMV_F_ROUTE_OUT) ||
                        (s.route_wt != KT_F32 && s.route_wt != KT_F16))
                        return -3;
                    p->ROUTE = 1;
                }
                p->waves = 8, cap = 256;
            } else if (mode == 0 && pro == 2 && rows <= 16384) {
                p->PF = 0, p->waves = 8, cap = 256;
            } else if (pro < 0 || pro > 3) {
                return -3;
            }
        }
    }
    if (!gemv_rows_split(s, p->R)) return -5;
    gemv_rs_grid(rows, s.K, cap, p);
    return 0;
}

inline int gemv_q4k_plan(const GemvShape &s, GemvPlan *p) {
    const int mode = s.mode, pro = s.pro;
    p->kernel = GEMV_Q4K;
    p->type = KT_Q4_K;
    if (s.nseg < 1 || s.nseg > 3) return -3;
    if (mode == 2 && (s.flags & (GEMV_F_EX | GEMV_F_NEOX))) return -3;
    p->mode = mode, p->pro = pro, p->PF = 0, p->waves = 4;
    if (s.K == 4096) {
        p->IT = 1, p->MC = 1;
        if (mode == 1 && pro == 1) p->R = 2, p->PF = 1;
        else if (mode == 2 && pro == 1) p->R = 2;
        else if (mode == 0 && pro == 0) p->R = 1;
        else if (mode == 0 && pro == 1) p->R = 2, p->PF = 1;
        else return -3;
    } else if (s.K == 14336 && mode == 0 && (pro == 2 || pro == 0)) {
        p->IT = 4, p->MC = 4, p->R = 1;
    } else {
        return -3;
    }
    if (!gemv_rows_split(s, p->R)) return -5;
    gemv_q4k_grid(gemv_rows(s), s.K, p);
    return 0;
}

inline int gemv_stream_plan(const GemvShape &s, GemvPlan *p) {
    p->kernel = GEMV_STREAM;
    p->type = KT_Q4_K;
    if (s.type != KT_Q4_K || s.K % 256 || s.nseg < 1 || s.nseg > 3 || (s.flags & GEMV_F_EID)) return -3;
    if (s.mode == 2 && (s.flags & (GEMV_F_EX | GEMV_F_NEOX))) return -3;
    if (s.K != 14336 || s.mode != 0 || s.pro != 2) return -3;
    p->mode = 0, p->pro = 2, p->LPR = 64, p->NI = 8, p->MC = 4, p->R = 1, p->waves = 4;
    if (!gemv_rows_split(s, 64 / p->LPR)) return -5;
    gemv_stream_grid(gemv_rows(s), s.K, p);
    return 0;
}

inline int gemv_unit_plan(const GemvShape &s, GemvPlan *p) {
    const int rpw = s.rows_per_wave;
    const int64_t mc = (s.K + 4095) / 4096;
    p->kernel = GEMV_UNIT;
    p->type = s.type;
    if (!gemv_unit_type(s.type)) return -3;
    p->waves = 4;
    if (s.mode == 2 || s.mode == 1) {
        if (s.pro != 1) return -7;
        p->mode = s.mode, p->pro = 1;
        p->R = s.mode == 2 || rpw >= 2 ? 2 : 1;
    } else {
        p->mode = 0, p->pro = s.pro == 0 || s.pro == 1 ? s.pro : 2;
        p->R = p->pro == 0 && rpw >= 4 ? 4 : (p->pro != 2 && rpw >= 2 ? 2 : 1);
    }
    p->MC = p->pro == 0 ? 1 : (p->pro == 1 ? (mc <= 1 ? 1 : 2) : (mc <= 2 ? 2 : (mc <= 4 ? 4 : 8)));
    const int64_t it = (s.K / gemv_unit_elems(s.type) + 63) / 64, it0 = p->pro == 2 ? 2 : 1;
    if (it > 4 * it0) return -8;
    p->IT = (int)(it <= it0 ? it0 : (it <= 2 * it0 ? 2 * it0 : 4 * it0));
    if (!gemv_rows_split(s, p->R)) return -5;
    if (p->pro != 0 && s.K > 4096 * p->MC) return -6;
    gemv_unit_grid(gemv_rows(s), s.K, p);
    return 0;
}

// what the entry runs for the shape; the return value is p->rc
inline int gemv_plan(const GemvShape &s, int entry, GemvPlan *p) {
    *p = GemvPlan{};
    // pro 3 (LayerNorm): instances of the RS kernels only
    if (s.pro == 3 && !((entry == GEMV_ENTRY_RS || entry == GEMV_ENTRY_DEC) && gemv_rs_type(s.type))) return p->rc = -3;
    switch (entry) {
    case GEMV_ENTRY_RS: p->rc = gemv_rs_plan(s, false, p); break;
    case GEMV_ENTRY_RS_AUX: p->rc = gemv_rs_plan(s, true, p); break;
    case GEMV_ENTRY_Q4K: p->rc = gemv_q4k_plan(s, p); break;
    case GEMV_ENTRY_STREAM: p->rc = gemv_stream_plan(s, p); break;
    case GEMV_ENTRY_UNIT: p->rc = gemv_unit_plan(s, p); break;
    default:
        if (gemv_rs_type(s.type)) {
            p->rc = gemv_rs_plan(s, false, p);
        } else if (s.mode == 2 && (s.flags & (GEMV_F_EX | GEMV_F_NEOX))) {
            p->kernel = GEMV_UNIT, p->rc = -3;
        } else {
            p->rc = s.type == KT_Q4_K ? gemv_q4k_plan(s, p) : -3;
            if (p->rc == -3) {
                *p = GemvPlan{};
                p->rc = gemv_unit_plan(s, p);
            }
        }
    }
    return p->rc;
}

// ---- the combined launches
// q|k (Q4_K_RS) + v (Q6_K_RS) in one grid (k_gemv_rs_qkv): the RS mode-2 launch's grid (R 2, 4 waves, cap 512) over all
// three segments; instances at K 4096 (Llama-3-8B), 8192 (Llama-3-70B) and 2048
struct GemvMixedPlan {
    int rc;
    int NIA, NIB, MC, EX;
    int PRO;                     // 1: rms_norm prologue, 3: LayerNorm (s.pro == 3; not with ex)
    int64_t nblk;
    int block;
    int64_t lds_bytes;
};
inline int gemv_qkv_mixed_plan(const GemvShape &s, GemvMixedPlan *m) {
    *m = GemvMixedPlan{};
    const bool ex = s.flags & (GEMV_F_EX | GEMV_F_NEOX);
    m->rc = -3;
    if (s.nseg != 3 || s.K % 256 || !gemv_rs_supported(KT_Q4_K_RS, s.K) || !gemv_rs_supported(KT_Q6_K_RS, s.K)) return m->rc;
    if (!gemv_rows_split(s, 2)) return m->rc = -5;
    // ex: segments 0, 1 = q, k and 2 = v as the runtime passes them; whole heads
    if (ex && (s.role[0] != 0 || s.role[1] != 1 || s.role[2] != 2)) return m->rc;
    if (ex && (s.flags & GEMV_F_NEOX) && (s.D < 2 || s.D % 2 || s.N[0] % s.D || s.N[1] % s.D)) return m->rc;
    if (s.pro == 3 && ex) return m->rc;
    m->PRO = s.pro == 3 ? 3 : 1;
    GemvPlan a{}, b{};
    gemv_rs_class(KT_Q4_K_RS, s.K, &a);
    gemv_rs_class(KT_Q6_K_RS, s.K, &b);
    if (!((a.NI == 2 && b.NI == 1 && a.MC == 1) || (a.NI == 4 && b.NI == 2 && a.MC == 2) || (a.NI == 1 && b.NI == 1 && a.MC == 1)))
        return m->rc;
    m->NIA = a.NI, m->NIB = b.NI, m->MC = a.MC, m->EX = ex;
    a.mode = 2, a.R = 2, a.waves = 4;
    gemv_rs_grid(gemv_rows(s), s.K, 512, &a);
    m->nblk = a.nblk, m->block = a.block, m->lds_bytes = a.lds_bytes;
    return m->rc = 0;
}

// q (an RS layout) + k|v (Q8_0) in one grid (k_gemv_qkv_dual): workgroups [0, a.nblk) are a's RS launch, the rest b's
// unit launch, each exactly its own plan, so the result is the two launches' bit for bit.  K <= 4096; instances at
// IT 2 (K > 2048) with NI 2 (Q4_K_RS, Q5_K_RS) or NI 1 (Q6_K_RS: K 4096)
struct GemvDualPlan {
    int rc;
    GemvPlan a, b;
    int64_t nblk;
    int64_t lds_bytes;
};
inline int gemv_qkv_dual_plan(GemvShape sa, GemvShape sb, GemvDualPlan *d) {
    *d = GemvDualPlan{};
    d->rc = -3;
    sa.mode = sb.mode = 2, sa.pro = sb.pro = 1;          // both halves: q|k|v with the norm prologue
    sb.type = KT_Q8_0, sb.rows_per_wave = 2;
    if (!gemv_rs_type(sa.type)) return d->rc;
    if (sa.K != sb.K || sa.K % 256 || sa.K > 4096 || !gemv_rs_supported(sa.type, sa.K) || (sa.flags & GEMV_F_ROUTE_W)) return d->rc;
    if ((sa.flags | sb.flags) & (GEMV_F_EX | GEMV_F_NEOX)) return d->rc;     // not in this grid: separate launches
    if (!gemv_rows_split(sa, 2) || !gemv_rows_split(sb, 2)) return d->rc = -5;
    if (gemv_plan(sa, GEMV_ENTRY_RS, &d->a) || gemv_plan(sb, GEMV_ENTRY_UNIT, &d->b)) return d->rc;
    if (d->b.IT != 2 || d->a.NI != (sa.type == KT_Q6_K_RS ? 1 : 2)) return d->rc;
    d->nblk = d->a.nblk + d->b.nblk;
    d->lds_bytes = std::max(d->a.lds_bytes, d->b.lds_bytes);
    return d->rc = 0;
}
