"""Generate tests/golden/grammar.npz: the reference's GBNF parser, stack set, per-step reject mask and accept step on
the grammars, the synthetic vocabulary and the token walks below (tests/test_grammar.py holds
koboldcpp_amd/csrc/grammar.h to it).

The reference's src/llama-grammar.cpp is compiled into a temporary directory behind tests/golden/grammar_driver.cpp,
which includes it as one translation unit (REF: the reference tree, default /root/reference as oracle/Makefile).  Run in
the build container only; the fixture holds data alone and is committed so the suite never needs the reference.

Per case i (a grammar and one walk): text_i, ok_i (0: the reference made no grammar of it), rules_i / rule_len_i (the
(type, value) element pairs rule after rule), stacks0_i (stacks after init), masks_i (one reject bitmask per step, taken
before the step's token), toks_i (the token accepted at each step) and state_i (per accepted token: stack count,
partial_utf8 value, n_remain).  The walk takes its forced tokens first, then a seeded choice among the allowed ones.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "grammar.npz")
REF = os.environ.get("REF", "/root/reference")

JSON = r'''# a JSON-like grammar
root   ::= value
value  ::= object | array | string | number | "true" | "false" | "null"
object ::= "{" ws ( pair ( "," ws pair )* )? "}"
pair   ::= string ws ":" ws value ws
array  ::= "[" ws ( value ws ( "," ws value ws )* )? "]"
string ::= "\"" ( [^"\\\x00-\x1f] | "\\" ( ["\\/bfnrt] | "u" [0-9a-fA-F]{4} ) )* "\""
number ::= "-"? ( "0" | [1-9] [0-9]* ) ( "." [0-9]+ )?
ws     ::= [ \t\n]*
'''

YESNO = 'root ::= ("yes" | "no") " " [0-9]{3}'

GRAMMARS = {
    "lit_alt": 'root ::= "yes" | "no" | "maybe" "\\n"',
    "nested": 'root ::= ("a" ("b" | "c" ("d" | "e"))) "!"   # groups in groups\n',
    "reps": 'root ::= "a"* "b"+ "c"? [0-9]{2} "x"{1,3} "y"{2,} "\\n"',
    "classes": 'root ::= [a-cX-Z0-9_]+ [^a-z\\n] . [^\\x00-\\x7f]? "."\n',
    "escapes": 'root ::= "\\t\\"\\\\" "\\x41\\u00e9\\U0001F600" [\\]\\[] "\\n"',
    "json": JSON,
    "yesno": YESNO,
    "empty_rule": 'root ::= ws "k" ws "k"\nws ::= | " " ws\n',
    "non_ascii": 'root ::= "h\u00e9llo" " " "\u65e5\u672c" "\U0001F600"? [\u3040-\u30ff]*',
    "multi_rule": 'root ::= item+\r\nitem ::= "- " word "\\n"\r\nword ::= [a-z]+ | [0-9]+\r\n',
    "bad_syntax": 'root ::= ("a" "b"',
    "bad_undefined": 'root ::= "a" thing',
    "bad_left_recursion": 'root ::= root "a" | "b"',
    "bad_left_recursion_nullable": 'root ::= opt root "a" | "b"\nopt ::= "x" |',
    "bad_no_root": 'start ::= "a"',
}


def vocab():
    v = [bytes([b]) for b in range(1, 128)]
    v += [b"ye", b"s\n", b'{"', b"yes", b"no", b"may", b"be\n", b"maybe", b" ", b"  ", b"true", b"fal", b"se", b"null",
          b'":', b'", "', b'"}', b"ab", b"abc", b"b!", b"ce!", b"aab", b"bb", b"xx", b"xy", b"yy", b"yyy", b"y\n", b"c1", b"- ",
          b"- a", b"z\n- ", b"\\u", b'\\"', b"[1", b", ", b"]]", b"0.5", b"-1", b"kk", b" k", b"k ", b"\t\"", b"\\A", b"A\xc3\xa9"]
    v += [b"%02d" % i for i in range(100)]
    # 2-, 3- and 4-byte characters whole and split, a piece that ends inside a character, one that starts inside one
    v += ["\u00e9".encode(), b"\xc3", b"\xa9", b"h\xc3", b"\xa9llo", "h\u00e9llo".encode(),
          "\u65e5".encode(), b"\xe6", b"\x97\xa5", b"\xe6\x97", b"\xa5", b"\x97", "\u672c".encode(), "\u65e5\u672c".encode(),
          b"\xe6\x9c", b"\xac", "\u3042".encode(), b"\xe3", b"\x81\x82", b"\xe3\x81", b"\x82",
          "\U0001F600".encode(), b"\xf0", b"\x9f\x98\x80", b"\xf0\x9f", b"\x98\x80", b"\xf0\x9f\x98", b"\x80", b"\x98", b"\x9f"]
    # invalid or overlong: a continuation byte as lead is above; 0xff / 0xf8 leads, overlong 2-byte forms, a lead cut short
    v += [b"\xff", b"\xf8\x88", b"\xc0\x80", b"\xc1", b"\xc0", b"a\x80", b"\xc3(", b"\xe6a"]
    v += [b"", b"\x00", b"\x00a"]                      # the empty piece; pieces that start with a zero byte
    eos = len(v)
    v += [b""]                                          # EOS renders as nothing
    return v, eos


def walks(name, v):
    """[(steps, seed, forced token ids)]"""
    ix = {p: i for i, p in enumerate(v)}
    f = lambda *ps: [ix[p] for p in ps]  # noqa: E731
    w = [(40, 1, []), (40, 2, [])]
    if name == "lit_alt":                             # an overlong U+0000 passes the mask and leaves no stack
        w += [(4, 11, f(b"\xc0\x80"))]
    if name == "json":
        w = [(64, s, []) for s in (1, 2, 3)] + [(40, 4, f(b'{"', b"a", b'":', b" ", b"[1", b", ", b"tr"[:1], b"r", b"u", b"e"))]
    if name == "yesno":
        w += [(8, 5, f(b"ye", b"s")), (8, 6, f(b"no", b" ", b"1", b"07"))]
    if name == "non_ascii":
        w += [(24, 7, f(b"h\xc3", b"\xa9llo", b" ", b"\xe6", b"\x97\xa5", b"\xe6\x9c", b"\xac", b"\xf0\x9f", b"\x98\x80", b"\xe3", b"\x81\x82")),
              (24, 8, f(b"h", b"\xc3", b"\xa9", b"l", b"l", b"o", b" ", b"\xe6\x97", b"\xa5", "\u672c".encode(), b"\xf0", b"\x9f\x98\x80",
                        b"\xe3\x81", b"\x82"))]
    if name == "escapes":
        w += [(12, 9, f(b"\t\"", b"\\A", b"\xc3", b"\xa9", b"\xf0\x9f\x98", b"\x80"))]
    if name == "classes":
        w += [(12, 10, f(b"ab", b"c1", b"_", b"X", b"\xe6", b"\x97\xa5", b"\xf0\x9f", b"\x98\x80", b"."))]
    return w


def main():
    v, eos = vocab()
    hx = lambda b: b.hex() if b else "-"  # noqa: E731
    job = ["V %d %d" % (len(v), eos)] + [hx(p) for p in v]
    cases = []
    for name, text in GRAMMARS.items():
        for steps, seed, forced in walks(name, v):
            job.append("G " + text.encode().hex())
            job.append("W %d %d %d %s" % (steps, seed, len(forced), " ".join(map(str, forced))))
            cases.append((name, text))
            if name.startswith("bad_"):
                break
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "grammar_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I%s/src" % REF, "-I%s/include" % REF, "-I%s/ggml/include" % REF,
                               os.path.join(HERE, "grammar_driver.cpp"), "-o", exe, "-Wl,--unresolved-symbols=ignore-all"])
        out = subprocess.run([exe], input="\n".join(job) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    nw = (len(v) + 31) // 32
    d = {"vocab_blob": np.frombuffer(b"".join(v), np.uint8), "vocab_off": np.cumsum([0] + [len(p) for p in v]).astype(np.int64),
         "eos": np.int32(eos), "n_cases": np.int32(len(cases)), "names": np.array([c[0] for c in cases])}
    at = 0
    for i, (name, text) in enumerate(cases):
        d["text_%d" % i] = np.frombuffer(text.encode(), np.uint8)
        if out[at] == "NOGRAMMAR":
            assert name.startswith("bad_"), (name, "the reference made no grammar of it")
            d["ok_%d" % i] = np.int32(0)
            at += 1
            continue
        assert not name.startswith("bad_"), name
        assert out[at].startswith("RULES "), out[at]
        nr = int(out[at].split()[1])
        at += 1
        elems, lens = [], []
        for _ in range(nr):
            t = out[at].split()
            assert t[0] == "R"
            lens.append(int(t[1]))
            elems += [int(x) for x in t[2:]]
            at += 1
        assert len(elems) == 2 * sum(lens)
        stacks0 = int(out[at].split()[1])
        at += 1
        masks, toks, state = [], [], []
        while out[at] != "END":
            t = out[at].split()
            assert t[0] != "ERR", out[at]
            if t[0] == "MASK":
                masks.append([int(x, 16) for x in t[1:]])
            elif t[0] == "TOK":
                toks.append(int(t[1]))
            elif t[0] == "STATE":
                state.append([int(x) for x in t[1:]])
            at += 1
        at += 1
        d["ok_%d" % i] = np.int32(1)
        d["rules_%d" % i] = np.array(elems, np.uint32)
        d["rule_len_%d" % i] = np.array(lens, np.int32)
        d["stacks0_%d" % i] = np.int32(stacks0)
        d["masks_%d" % i] = np.array(masks, np.uint32).reshape(len(masks), nw)
        d["toks_%d" % i] = np.array(toks, np.int32)
        d["state_%d" % i] = np.array(state, np.int64).reshape(len(toks), 3)
        print("%-12s rules %3d stacks %3d steps %3d tokens %s" % (name, nr, stacks0, len(masks), toks[:12]))
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
