"""Generate tests/golden/commandr_tiny.npz: the tiny Command-R models (tests/commandr_gguf.py TINY_CMDR) through the
REFERENCE ggml, driven over ctypes as make_qwen2.py does (oracle/_ref/libggml_ref.so and the scalar build of `make -C
oracle ref_scalar`).  Run in the build container only; the fixture is committed so the suites never need the reference
sources.

The graph is build_command_r's node sequence (src/llama.cpp:13986-14133; the tensors at :8247-8285): per layer ggml_norm
* attn_norm (LLM_NORM, no bias), mul_mat for q / k / v, ggml_rope_ext mode 0 (NORM pairs), the f16 K / V cache copies,
ggml_flash_attn_ext under llama.cpp's padded f16 mask (or llm_build_kqv's other branch with flash attention off), wo;
the SiLU-GLU FFN on the SAME normalised rows; (ffn_out + x) + attn_out; then ggml_norm * output_norm, the head over the
tied token embedding and ggml_scale by logit_scale.

Per tag (commandr_gguf.TAGS): types, prompt, the reference's greedy tokens, the AVX2 build's logits per step, the
per-step max / median |dlogit| between the AVX2 and scalar builds ("spread") and between the flash-attention graph and
the flash-attention-off graph ("fagap"), and |mean| / std of every layer's input rows for the prompt ("lin_ms").
For KVQ_TAG also the flash-attention graph over a Q8_0 K / V cache (llama_context_params type_k / type_v; koboldcpp
--quantkv 1): kvq8_logits and its own AVX2-vs-scalar spread.
Beside them ln_x / ln_w / ln_y per LN_CASES entry: rows with means up to 3 x their std through ggml_norm + ggml_mul.

The prompt seed is stepped until, for every tag, the top-2 logit margin of at least 4 of the 7 steps exceeds
4 x max(spread_max, fagap_max) (those steps pin the greedy token); the seed is stored.  The script also asserts that
every tag has layer-input rows with |mean| / std >= 0.25 in both layers, so that LayerNorm cannot pass for RMS norm.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import commandr_gguf as C  # noqa: E402
import make_qwen2 as MQ  # noqa: E402
import refharness as R  # noqa: E402

OUT = os.path.join(HERE, "commandr_tiny.npz")
I32 = 26                 # GGML_TYPE_I32
ROPE_NORM = 0
LN_EPS = 1e-5
LN_CASES = {"ln2048": (2048, 1), "ln1792": (1792, 9), "ln8192": (8192, 3)}     # name: (width, rows)
MIN_MS, MIN_PINNED, MARGIN_X = 0.25, 4, 4.0
KVQ_TAG = "q4km"


class Ggml(MQ.Ggml):
    def __init__(self, path):
        super().__init__(path)
        P, F = ctypes.c_void_p, ctypes.c_float
        for n, (res, args) in {"ggml_norm": (P, [P, P, F]), "ggml_scale": (P, [P, P, F])}.items():
            fn = getattr(self.L, n)
            fn.restype, fn.argtypes = res, args
            setattr(self, n[5:], fn)


def ln_case_inputs(name):
    """x [rows][width] f32: bell-shaped multiples of 2^-16 (std 0.58) plus a row constant between -3 and 3 times that
    std (the subtraction of the mean cancels digits); w [width]: 1 + bell / 2^19 (about 1 +- 0.07)"""
    import zlib
    width, rows = LN_CASES[name]
    seed = zlib.crc32(name.encode())
    x = (R._hash_bell(seed, 1, rows * width).astype(np.float64) / 65536.0).reshape(rows, width)
    k = np.linspace(-3.0, 3.0, rows) if rows > 1 else np.array([3.0])
    x = (x + (0.58 * k)[:, None]).astype(np.float32)
    w = (1.0 + R._hash_bell(seed, 2, width).astype(np.float64) / 524288.0).astype(np.float32)
    return x, w


def ln_cases(g):
    out = {}
    for name, (width, rows) in LN_CASES.items():
        x, w = ln_case_inputs(name)
        ctx = g.ctx(rows * width * 16 + (1 << 20))
        tx = g.new_tensor_2d(ctx, R.F32, width, rows)
        g.put(tx, x)
        tw = g.new_tensor_1d(ctx, R.F32, width)
        g.put(tw, w)
        y = g.mul(ctx, g.norm(ctx, tx, LN_EPS), tw)
        gf = g.new_graph_custom(ctx, 64, False)
        g.build_forward_expand(gf, y)
        assert g.graph_compute_with_ctx(ctx, gf, MQ.NTHREADS) == 0
        out[name + "_x"], out[name + "_w"] = x, w
        out[name + "_y"] = g.get(y, np.float32, rows * width).reshape(rows, width)
        g.free(ctx)
    return out


class RefCommandR:
    def __init__(self, g, hp, types, fa, kvt=R.F16):
        self.g, self.hp, self.fa, self.kvt = g, hp, fa, kvt
        assert fa or kvt == R.F16                             # a quantized cache implies flash attention
        E = hp["n_embd"]
        self.D = E // hp["n_head"]
        self.EKV = hp["n_head_kv"] * self.D
        shapes = R.weight_shapes(hp)
        total = sum(R.row_bytes(t, k) * n + 256 for (k, n), t in zip(shapes, types))
        total += hp["n_layer"] * (2 * self.EKV * hp["n_ctx"] * 2 + 5 * 256)       # (a Q8_0 cache is smaller)
        total += (len(shapes) + 8 * hp["n_layer"] + 16) * g.tensor_overhead()
        self.wctx = g.ctx(total)
        self.w = []
        for idx, ((k, n), t) in enumerate(zip(shapes, types)):
            w = g.new_tensor_2d(self.wctx, t, k, n)
            g.put(w, C.embedding_bytes(hp) if idx in (0, 2) else
                  (C.output_norm_f32(hp) if idx == 1 else R.synth_tensor(hp, t, C.SEED, idx)))
            self.w.append(w)
        self.kc, self.vc = [], []
        for il in range(hp["n_layer"]):
            for lst in (self.kc, self.vc):
                c = g.new_tensor_1d(self.wctx, kvt, self.EKV * hp["n_ctx"])
                g.put(c, np.zeros(R.row_bytes(kvt, self.EKV) * hp["n_ctx"], np.uint8))
                lst.append(c)

    def rope(self, ctx, x, pos):
        hp = self.hp
        return self.g.rope_ext(ctx, x, pos, None, self.D, ROPE_NORM, hp["n_ctx"], hp["rope_base"], 1.0, 0.0, 1.0, 32.0, 1.0)

    def eval(self, tokens, n_past):
        """logits of the last token, and |mean| / std of each layer's input rows [n_layer][T]"""
        g, hp = self.g, self.hp
        E, H, HKV, D, EKV, F = hp["n_embd"], hp["n_head"], hp["n_head_kv"], self.D, self.EKV, hp["n_ff"]
        T = len(tokens)
        n_kv = n_past + T
        T_pad = (T + MQ.KQ_MASK_PAD - 1) // MQ.KQ_MASK_PAD * MQ.KQ_MASK_PAD
        mem = T * hp["n_layer"] * (E * 20 + F * 4 + EKV * 8 + H * n_kv * 3) * 4 + n_kv * T_pad * 4 + hp["n_vocab"] * 8 \
            + (hp["n_layer"] * 80 + 64) * g.tensor_overhead() + g.graph_overhead_custom(8192, False) + (64 << 20)
        ctx = g.ctx(mem)
        gf = g.new_graph_custom(ctx, 8192, False)
        inp_tokens = g.new_tensor_1d(ctx, I32, T)
        g.put(inp_tokens, np.asarray(tokens, np.int32))
        inp_pos = g.new_tensor_1d(ctx, I32, T)
        g.put(inp_pos, np.arange(n_past, n_past + T, dtype=np.int32))
        m = np.full((T_pad, n_kv), -np.inf, np.float32)
        for t in range(T):
            m[t, :n_past + t + 1] = 0.0
        kq_mask = g.new_tensor_2d(ctx, R.F16 if self.fa else R.F32, n_kv, T_pad)
        g.put(kq_mask, m.astype(np.float16) if self.fa else m)
        inp_out = g.new_tensor_1d(ctx, I32, 1)
        g.put(inp_out, np.array([T - 1], np.int32))
        kq_scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        esz, kvt = 2, self.kvt
        inpL = g.get_rows(ctx, self.w[0], inp_tokens)
        lin = []
        for il in range(hp["n_layer"]):
            lw = self.w[3 + 9 * il: 12 + 9 * il]
            lin.append(inpL)
            cur = g.mul(ctx, g.norm(ctx, inpL, hp["eps"]), lw[0])
            ffn_inp = cur
            Qcur = g.mul_mat(ctx, lw[1], cur)
            Kcur = g.mul_mat(ctx, lw[2], cur)
            Vcur = g.mul_mat(ctx, lw[3], cur)
            Qcur = self.rope(ctx, g.reshape_3d(ctx, Qcur, D, H, T), inp_pos)
            Kcur = self.rope(ctx, g.reshape_3d(ctx, Kcur, D, HKV, T), inp_pos)
            kview = g.view_1d(ctx, self.kc[il], T * EKV, g.row_size(kvt, EKV) * n_past)
            g.build_forward_expand(gf, g.cpy(ctx, Kcur, kview))
            if self.fa:
                vview = g.view_1d(ctx, self.vc[il], T * EKV, g.row_size(kvt, EKV) * n_past)
                g.build_forward_expand(gf, g.cpy(ctx, g.reshape_2d(ctx, Vcur, EKV, T), vview))
            else:
                vview = g.view_2d(ctx, self.vc[il], T, EKV, hp["n_ctx"] * esz, n_past * esz)
                g.build_forward_expand(gf, g.cpy(ctx, g.transpose(ctx, g.reshape_2d(ctx, Vcur, EKV, T)), vview))
            q = g.permute(ctx, Qcur, 0, 2, 1, 3)
            k = g.view_3d(ctx, self.kc[il], D, n_kv, HKV, g.row_size(kvt, EKV), g.row_size(kvt, D), 0)
            if self.fa:
                v = g.view_3d(ctx, self.vc[il], D, n_kv, HKV, g.row_size(kvt, EKV), g.row_size(kvt, D), 0)
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
                inpL = g.get_rows(ctx, inpL, inp_out)
                ffn_inp = g.get_rows(ctx, ffn_inp, inp_out)
            attn_out = cur
            up = g.mul_mat(ctx, lw[7], ffn_inp)               # llm_build_ffn, LLM_FFN_SILU / LLM_FFN_PAR
            gate = g.mul_mat(ctx, lw[6], ffn_inp)
            cur = g.mul_mat(ctx, lw[8], g.mul(ctx, g.silu(ctx, gate), up))
            cur = g.add(ctx, cur, inpL)
            inpL = g.add(ctx, cur, attn_out)
        cur = g.mul(ctx, g.norm(ctx, inpL, hp["eps"]), self.w[1])
        cur = g.mul_mat(ctx, self.w[2], cur)
        cur = g.scale(ctx, cur, hp["logit_scale"])
        g.build_forward_expand(gf, cur)
        assert g.graph_compute_with_ctx(ctx, gf, MQ.NTHREADS) == 0
        logits = g.get(cur, np.float32, hp["n_vocab"])
        ms = []
        for t in lin:
            x = g.get(t, np.float32, T * E).reshape(T, E).astype(np.float64)
            ms.append(np.abs(x.mean(axis=1)) / x.std(axis=1))
        g.free(ctx)
        return logits, np.stack(ms).astype(np.float32)


def run(lib, tag, fa, pseed, forced=None, ln=False, kvt=R.F16):
    g = Ggml(lib)
    hp = C.tag_hp(tag)
    m = RefCommandR(g, hp, C.tag_types(tag), fa, kvt)
    prompt = C.prompt_tokens(hp, pseed)
    lg, ms = m.eval(prompt, 0)
    logits, toks, n = [lg], [], len(prompt)
    for i in range(C.N_GEN):
        tok = int(forced[i]) if forced is not None else int(np.argmax(logits[-1]))
        toks.append(tok)
        logits.append(m.eval([tok], n)[0])
        n += 1
    out = dict(logits=np.stack(logits), tokens=np.array(toks, np.int32), lin_ms=ms)
    if ln:
        out.update(ln_cases(g))
    return out


def run_child(lib, tag, fa, pseed, forced=None, ln=False, kvt=R.F16):
    with tempfile.TemporaryDirectory() as td:
        o = os.path.join(td, "o.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", lib, tag, str(int(fa)), o, str(pseed), str(int(ln)), str(kvt)]
        if forced is not None:
            cmd.append(",".join(str(int(t)) for t in forced))
        subprocess.check_call(cmd)
        return dict(np.load(o))


def pinned_steps(logits, bar):
    """the steps whose top-2 logit margin exceeds bar"""
    top2 = np.sort(logits.astype(np.float64), axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > bar


def attempt(pseed):
    fx = {"prompt_seed": np.array(pseed, np.int32)}
    for tag in C.TAGS:
        a = run_child(MQ.REFLIB, tag, True, pseed, ln=tag == C.TAGS[0])
        toks = a["tokens"]
        s = run_child(MQ.REFLIB_SCALAR, tag, True, pseed, forced=toks)
        f = run_child(MQ.REFLIB, tag, False, pseed, forced=toks)
        fx[tag + "_types"] = np.array(C.tag_types(tag), np.int32)
        fx[tag + "_prompt"] = np.array(C.prompt_tokens(C.tag_hp(tag), pseed), np.int32)
        fx[tag + "_tokens"] = toks
        fx[tag + "_logits"] = a["logits"]
        fx[tag + "_lin_ms"] = a["lin_ms"]
        for nm, b in (("spread", s), ("fagap", f)):
            d = np.abs(a["logits"].astype(np.float64) - b["logits"].astype(np.float64))
            fx["%s_%s_max" % (tag, nm)] = d.max(axis=1).astype(np.float32)
            fx["%s_%s_med" % (tag, nm)] = np.median(d, axis=1).astype(np.float32)
        fx.update({k: v for k, v in a.items() if k.startswith("ln")})
        bar = MARGIN_X * max(float(fx[tag + "_spread_max"].max()), float(fx[tag + "_fagap_max"].max()))
        npin = int(pinned_steps(a["logits"], bar).sum())
        ms = a["lin_ms"]
        print(tag, "seed", pseed, "tokens", toks.tolist(), "spread max", fx[tag + "_spread_max"].max(), "fagap max",
              fx[tag + "_fagap_max"].max(), "pinned", npin, "lin |mean|/std max per layer", ms.max(axis=1))
        assert (ms.max(axis=1) >= MIN_MS).all(), "layer-input rows are too close to zero mean"
        if npin < MIN_PINNED:
            return None
        if tag == KVQ_TAG:
            qa = run_child(MQ.REFLIB, tag, True, pseed, forced=toks, kvt=R.Q8_0)
            qs = run_child(MQ.REFLIB_SCALAR, tag, True, pseed, forced=toks, kvt=R.Q8_0)
            d = np.abs(qa["logits"].astype(np.float64) - qs["logits"].astype(np.float64))
            fx["kvq8_logits"] = qa["logits"]
            fx["kvq8_spread_max"], fx["kvq8_spread_med"] = d.max(axis=1).astype(np.float32), np.median(d, axis=1).astype(np.float32)
            print(tag, "Q8_0 cache: spread max", d.max(), "vs the f16 cache", np.abs(qa["logits"] - a["logits"]).max())
    return fx


def main():
    for pseed in range(C.SEED, C.SEED + 64):
        fx = attempt(pseed)
        if fx is not None:
            break
    else:
        raise SystemExit("no prompt seed pins %d steps in every tag" % MIN_PINNED)
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        lib, tag, fa, o, pseed, ln, kvt = sys.argv[2:9]
        forced = [int(t) for t in sys.argv[9].split(",")] if len(sys.argv) > 9 else None
        np.savez(o, **run(lib, tag, bool(int(fa)), int(pseed), forced=forced, ln=bool(int(ln)), kvt=int(kvt)))
    else:
        main()
