"""Generate tests/golden/qwen2_tiny.npz: the tiny Qwen2 models (tests/qwen2_gguf.py TINY_QWEN2, WIDE_QWEN2) through the REFERENCE
ggml, driven over ctypes (oracle/_ref/libggml_ref.so, and the scalar build of `make -C oracle ref_scalar`).  Run in the
build container only; the fixture is committed so the suites never need the reference sources.

The graph is build_qwen2's node sequence (src/llama.cpp:12136-12246; the tensors at :7739-7777): rms_norm * w, mul_mat +
f32 bias add for q / k / v, ggml_rope_ext mode 2 (NeoX), the f16 K / V cache copies, ggml_flash_attn_ext under
llama.cpp's padded f16 mask, wo, residual, norm, SiLU-GLU FFN, output norm and head -- or, with flash attention off,
llm_build_kqv's other branch (mul_mat, soft_max_ext under the f32 mask, the transposed V cache).  The prompt is one
batch, every later token a batch of one over the cache, as llama.cpp evaluates them (the CPU mat-mul route depends on
the batch size, sgemm.cpp:1033).

Per tag (qwen2_gguf.TAGS) the fixture holds: types, prompt, the reference's greedy tokens (the teacher-forced ones),
the AVX2 build's logits per step, the per-step max / median |dlogit| between the AVX2 and scalar builds ("spread"), the
same between the flash-attention graph and the flash-attention-off graph ("fagap": the reference's own f16-versus-f32
accumulation gap), and for q4km a NeoX K-shift case (layer 0's cache rows before, (p0, diff), the rows after).
Beside them: ggml_rope_ext mode 2 of hashed q / k rows (qwen2_gguf.ROPE_CASES: head dims 128 and 64) for the rope kernels' test.

Each (build, graph) runs in a process of its own: the two builds export the same symbols.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import qwen2_gguf as Q  # noqa: E402
import refharness as R  # noqa: E402

REFLIB = os.path.join(R.ROOT, "oracle", "_ref", "libggml_ref.so")
REFLIB_SCALAR = os.path.join(R.ROOT, "oracle", "_ref", "scalar", "libggml_ref.so")
OUT = os.path.join(HERE, "qwen2_tiny.npz")
KSHIFT = (3, 5)          # (p0, diff) of the K-shift case
NTHREADS = 4
ROPE_NEOX = 2            # GGML_ROPE_TYPE_NEOX
KQ_MASK_PAD = 32         # GGML_KQ_MASK_PAD


class Ggml:
    """the few graph-API entry points of the reference ggml this generator needs"""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        P, I, I64, F, SZ, B = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t, ctypes.c_bool

        class InitParams(ctypes.Structure):
            _fields_ = [("mem_size", SZ), ("mem_buffer", P), ("no_alloc", B)]
        self.InitParams = InitParams
        sig = {
            "ggml_init": (P, [InitParams]), "ggml_free": (None, [P]), "ggml_get_data": (P, [P]), "ggml_nbytes": (SZ, [P]),
            "ggml_tensor_overhead": (SZ, []), "ggml_graph_overhead_custom": (SZ, [SZ, B]),
            "ggml_row_size": (SZ, [I, I64]),
            "ggml_new_tensor_1d": (P, [P, I, I64]), "ggml_new_tensor_2d": (P, [P, I, I64, I64]),
            "ggml_new_tensor_3d": (P, [P, I, I64, I64, I64]),
            "ggml_new_graph_custom": (P, [P, SZ, B]), "ggml_build_forward_expand": (None, [P, P]),
            "ggml_graph_compute_with_ctx": (I, [P, P, I]),
            "ggml_get_rows": (P, [P, P, P]), "ggml_mul": (P, [P, P, P]), "ggml_add": (P, [P, P, P]),
            "ggml_mul_mat": (P, [P, P, P]), "ggml_rms_norm": (P, [P, P, F]), "ggml_silu": (P, [P, P]),
            "ggml_reshape_2d": (P, [P, P, I64, I64]), "ggml_reshape_3d": (P, [P, P, I64, I64, I64]),
            "ggml_rope_ext": (P, [P, P, P, P, I, I, I, F, F, F, F, F, F]),
            "ggml_rope_ext_inplace": (P, [P, P, P, P, I, I, I, F, F, F, F, F, F]),
            "ggml_view_1d": (P, [P, P, I64, SZ]), "ggml_view_2d": (P, [P, P, I64, I64, SZ, SZ]),
            "ggml_view_3d": (P, [P, P, I64, I64, I64, SZ, SZ, SZ]),
            "ggml_cpy": (P, [P, P, P]), "ggml_permute": (P, [P, P, I, I, I, I]), "ggml_transpose": (P, [P, P]),
            "ggml_cont_2d": (P, [P, P, I64, I64]),
            "ggml_flash_attn_ext": (P, [P, P, P, P, P, F, F, F]), "ggml_soft_max_ext": (P, [P, P, P, F, F]),
        }
        for n, (res, args) in sig.items():
            fn = getattr(L, n)
            fn.restype, fn.argtypes = res, args
            setattr(self, n[5:], fn)

    def ctx(self, nbytes):
        c = self.init(self.InitParams(nbytes, None, False))
        assert c
        return c

    def put(self, t, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes(t), (arr.nbytes, self.nbytes(t))
        ctypes.memmove(self.get_data(t), arr.ctypes.data, arr.nbytes)

    def get(self, t, dtype, count):
        out = np.empty(count, dtype)
        ctypes.memmove(out.ctypes.data, self.get_data(t), out.nbytes)
        return out


class RefQwen2:
    def __init__(self, g, hp, types, fa):
        self.g, self.hp, self.fa = g, hp, fa
        E = hp["n_embd"]
        self.D = E // hp["n_head"]
        self.EKV = hp["n_head_kv"] * self.D
        shapes = R.weight_shapes(hp)
        total = sum(R.row_bytes(t, k) * n + 256 for (k, n), t in zip(shapes, types))
        total += hp["n_layer"] * (2 * self.EKV * hp["n_ctx"] * 2 + (E + 2 * self.EKV) * 4 + 5 * 256)
        total += (len(shapes) + 8 * hp["n_layer"] + 16) * g.tensor_overhead()
        self.wctx = g.ctx(total)
        self.w = []
        for idx, ((k, n), t) in enumerate(zip(shapes, types)):
            w = g.new_tensor_2d(self.wctx, t, k, n)
            g.put(w, R.synth_tensor(hp, t, Q.SEED, idx))
            self.w.append(w)
        self.bias, self.kc, self.vc = [], [], []
        for il in range(hp["n_layer"]):
            bs = []
            for b in Q.qkv_bias(hp, il):
                t = g.new_tensor_1d(self.wctx, R.F32, len(b))
                g.put(t, b)
                bs.append(t)
            self.bias.append(bs)
            for lst in (self.kc, self.vc):
                c = g.new_tensor_1d(self.wctx, R.F16, self.EKV * hp["n_ctx"])
                g.put(c, np.zeros(self.EKV * hp["n_ctx"], np.uint16))
                lst.append(c)

    def rope(self, ctx, x, pos, inplace=False):
        hp = self.hp
        fn = self.g.rope_ext_inplace if inplace else self.g.rope_ext
        return fn(ctx, x, pos, None, self.D, ROPE_NEOX, hp["n_ctx"], hp["rope_base"], hp.get("rope_freq_scale", 1.0),
                  0.0, 1.0, 32.0, 1.0)

    def eval(self, tokens, n_past):
        g, hp = self.g, self.hp
        E, H, HKV, D, EKV, F = hp["n_embd"], hp["n_head"], hp["n_head_kv"], self.D, self.EKV, hp["n_ff"]
        T = len(tokens)
        n_kv = n_past + T
        T_pad = (T + KQ_MASK_PAD - 1) // KQ_MASK_PAD * KQ_MASK_PAD
        mem = T * hp["n_layer"] * (E * 16 + F * 4 + EKV * 8 + H * n_kv * 3) * 4 + n_kv * T_pad * 4 + hp["n_vocab"] * 8 \
            + (hp["n_layer"] * 80 + 64) * g.tensor_overhead() + g.graph_overhead_custom(8192, False) + (64 << 20)
        ctx = g.ctx(mem)
        gf = g.new_graph_custom(ctx, 8192, False)
        inp_tokens = g.new_tensor_1d(ctx, 26, T)             # GGML_TYPE_I32
        g.put(inp_tokens, np.asarray(tokens, np.int32))
        inp_pos = g.new_tensor_1d(ctx, 26, T)
        g.put(inp_pos, np.arange(n_past, n_past + T, dtype=np.int32))
        m = np.full((T_pad, n_kv), -np.inf, np.float32)
        for t in range(T):
            m[t, :n_past + t + 1] = 0.0
        kq_mask = g.new_tensor_2d(ctx, R.F16 if self.fa else R.F32, n_kv, T_pad)
        g.put(kq_mask, m.astype(np.float16) if self.fa else m)
        inp_out = g.new_tensor_1d(ctx, 26, 1)
        g.put(inp_out, np.array([T - 1], np.int32))
        kq_scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        esz = 2                                               # f16 cache element
        inpL = g.get_rows(ctx, self.w[0], inp_tokens)
        for il in range(hp["n_layer"]):
            lw = self.w[3 + 9 * il: 12 + 9 * il]
            bq, bk, bv = self.bias[il]
            inpSA = inpL
            cur = g.mul(ctx, g.rms_norm(ctx, inpL, hp["eps"]), lw[0])
            Qcur = g.add(ctx, g.mul_mat(ctx, lw[1], cur), bq)
            Kcur = g.add(ctx, g.mul_mat(ctx, lw[2], cur), bk)
            Vcur = g.add(ctx, g.mul_mat(ctx, lw[3], cur), bv)
            Qcur = self.rope(ctx, g.reshape_3d(ctx, Qcur, D, H, T), inp_pos)
            Kcur = self.rope(ctx, g.reshape_3d(ctx, Kcur, D, HKV, T), inp_pos)
            # llm_build_kv_store (src/llama.cpp:9180-9202)
            kview = g.view_1d(ctx, self.kc[il], T * EKV, g.row_size(R.F16, EKV) * n_past)
            g.build_forward_expand(gf, g.cpy(ctx, Kcur, kview))
            if self.fa:
                vview = g.view_1d(ctx, self.vc[il], T * EKV, g.row_size(R.F16, EKV) * n_past)
                g.build_forward_expand(gf, g.cpy(ctx, g.reshape_2d(ctx, Vcur, EKV, T), vview))
            else:                                             # the V cache is transposed without flash attention
                vview = g.view_2d(ctx, self.vc[il], T, EKV, hp["n_ctx"] * esz, n_past * esz)
                g.build_forward_expand(gf, g.cpy(ctx, g.transpose(ctx, g.reshape_2d(ctx, Vcur, EKV, T)), vview))
            # llm_build_kqv (src/llama.cpp:9517-9634)
            q = g.permute(ctx, Qcur, 0, 2, 1, 3)
            k = g.view_3d(ctx, self.kc[il], D, n_kv, HKV, g.row_size(R.F16, EKV), g.row_size(R.F16, D), 0)
            if self.fa:
                v = g.view_3d(ctx, self.vc[il], D, n_kv, HKV, g.row_size(R.F16, EKV), g.row_size(R.F16, D), 0)
                cur = g.flash_attn_ext(ctx, q, k, v, kq_mask, kq_scale, 0.0, 0.0)
                cur = g.reshape_2d(ctx, cur, E, T)
            else:
                kq = g.soft_max_ext(ctx, g.mul_mat(ctx, k, q), kq_mask, kq_scale, 0.0)
                v = g.view_3d(ctx, self.vc[il], n_kv, D, HKV, esz * hp["n_ctx"], esz * hp["n_ctx"] * D, 0)
                kqv = g.mul_mat(ctx, v, kq)
                cur = g.cont_2d(ctx, g.permute(ctx, kqv, 0, 2, 1, 3), E, T)
            cur = g.mul_mat(ctx, lw[4], cur)
            if il == hp["n_layer"] - 1:                       # skip unused tokens in the last layer
                cur = g.get_rows(ctx, cur, inp_out)
                inpSA = g.get_rows(ctx, inpSA, inp_out)
            ffn_inp = g.add(ctx, cur, inpSA)
            cur = g.mul(ctx, g.rms_norm(ctx, ffn_inp, hp["eps"]), lw[5])
            up = g.mul_mat(ctx, lw[7], cur)
            gate = g.mul_mat(ctx, lw[6], cur)
            cur = g.mul_mat(ctx, lw[8], g.mul(ctx, g.silu(ctx, gate), up))
            inpL = g.add(ctx, cur, ffn_inp)
        cur = g.mul(ctx, g.rms_norm(ctx, inpL, hp["eps"]), self.w[1])
        cur = g.mul_mat(ctx, self.w[2], cur)
        g.build_forward_expand(gf, cur)
        assert g.graph_compute_with_ctx(ctx, gf, NTHREADS) == 0
        logits = g.get(cur, np.float32, hp["n_vocab"])
        g.free(ctx)
        return logits

    def k_rows(self, il, lo, hi):
        return self.g.get(self.kc[il], np.uint16, self.EKV * self.hp["n_ctx"]).reshape(-1, self.EKV)[lo:hi].copy()

    def kshift_rows(self, rows, diff):
        """build_k_shift (src/llama.cpp:10144-10190) on cache rows [n][EKV] f16: ggml_rope_ext_inplace, NeoX, position
        -diff"""
        g = self.g
        n = rows.shape[0]
        ctx = g.ctx(n * self.EKV * 16 + (1 << 20))
        k = g.new_tensor_3d(ctx, R.F16, self.D, self.hp["n_head_kv"], n)
        g.put(k, rows)
        pos = g.new_tensor_1d(ctx, 26, n)
        g.put(pos, np.full(n, -diff, np.int32))
        r = self.rope(ctx, k, pos, inplace=True)
        gf = g.new_graph_custom(ctx, 64, False)
        g.build_forward_expand(gf, r)
        assert g.graph_compute_with_ctx(ctx, gf, NTHREADS) == 0
        out = g.get(r, np.uint16, n * self.EKV).reshape(n, self.EKV)
        g.free(ctx)
        return out


def rope_cases(g, hp):
    """ggml_rope_ext mode 2 of the q and k parts of each case: name_q [T][H][D], name_k [T][HKV][D]"""
    out = {}
    for name, (T, H, HKV, D, pos) in Q.ROPE_CASES.items():
        x = Q.rope_case_input(name)
        for part, lo, nh in (("q", 0, H), ("k", H * D, HKV)):
            ctx = g.ctx((T * nh * D * 16) + (1 << 20))
            t = g.new_tensor_3d(ctx, R.F32, D, nh, T)
            g.put(t, x[:, lo:lo + nh * D])
            p = g.new_tensor_1d(ctx, 26, T)
            g.put(p, np.asarray(pos, np.int32))
            r = g.rope_ext(ctx, t, p, None, D, ROPE_NEOX, hp["n_ctx"], hp["rope_base"], 1.0, 0.0, 1.0, 32.0, 1.0)
            gf = g.new_graph_custom(ctx, 64, False)
            g.build_forward_expand(gf, r)
            assert g.graph_compute_with_ctx(ctx, gf, NTHREADS) == 0
            out["%s_%s" % (name, part)] = g.get(r, np.float32, T * nh * D).reshape(T, nh, D)
            g.free(ctx)
    return out


def run(lib, tag, fa, forced=None, steps=None, kshift=False):
    """logits [1 + N_GEN][n_vocab] of the prompt and N_GEN single-token steps (greedy, or teacher-forced);
    steps: only that many rows (the pin test regenerates one)"""
    g = Ggml(lib)
    hp = Q.tag_hp(tag)
    m = RefQwen2(g, hp, Q.tag_types(tag), fa)
    prompt = Q.prompt_tokens(hp)
    logits = [m.eval(prompt, 0)]
    toks = []
    n = len(prompt)
    for i in range(Q.N_GEN if steps is None else steps - 1):
        tok = int(forced[i]) if forced is not None else int(np.argmax(logits[-1]))
        toks.append(tok)
        logits.append(m.eval([tok], n))
        n += 1
    out = dict(logits=np.stack(logits), tokens=np.array(toks, np.int32))
    if kshift:
        p0, diff = KSHIFT
        before = m.k_rows(0, p0 + diff, n)
        out.update(kshift_before=before, kshift_after=m.kshift_rows(before, diff))
        out.update(rope_cases(g, hp))
    return out


def run_child(lib, tag, fa, forced=None, kshift=False):
    with tempfile.TemporaryDirectory() as td:
        o = os.path.join(td, "o.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", lib, tag, str(int(fa)), o, str(int(kshift))]
        if forced is not None:
            cmd.append(",".join(str(int(t)) for t in forced))
        subprocess.check_call(cmd)
        return dict(np.load(o))


def main():
    fx = {"kshift_p0_diff": np.array(KSHIFT, np.int32)}
    for tag in Q.TAGS:
        a = run_child(REFLIB, tag, True, kshift=tag == "q4km")
        toks = a["tokens"]
        s = run_child(REFLIB_SCALAR, tag, True, forced=toks)
        f = run_child(REFLIB, tag, False, forced=toks)
        fx[tag + "_types"] = np.array(Q.tag_types(tag), np.int32)
        fx[tag + "_prompt"] = np.array(Q.prompt_tokens(Q.tag_hp(tag)), np.int32)
        fx[tag + "_tokens"] = toks
        fx[tag + "_logits"] = a["logits"]
        for nm, b in (("spread", s), ("fagap", f)):
            d = np.abs(a["logits"].astype(np.float64) - b["logits"].astype(np.float64))
            fx["%s_%s_max" % (tag, nm)] = d.max(axis=1).astype(np.float32)
            fx["%s_%s_med" % (tag, nm)] = np.median(d, axis=1).astype(np.float32)
        if "kshift_before" in a:
            fx["kshift_before"], fx["kshift_after"] = a["kshift_before"], a["kshift_after"]
            fx.update({k: v for k, v in a.items() if k.startswith("rope")})
        print(tag, "tokens", toks.tolist(), "spread max", fx[tag + "_spread_max"].max(), "fagap max", fx[tag + "_fagap_max"].max())
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        lib, tag, fa, o, ks = sys.argv[2:7]
        forced = [int(t) for t in sys.argv[7].split(",")] if len(sys.argv) > 7 else None
        np.savez(o, **run(lib, tag, bool(int(fa)), forced=forced, kshift=bool(int(ks))))
    else:
        main()
