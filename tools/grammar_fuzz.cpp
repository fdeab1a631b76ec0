// grammar_fuzz -- koboldcpp_amd/csrc/grammar.h under the host sanitizers: a stand-alone program (never loaded into
// Python, never run on a GPU machine) that pushes the grammars of tests/golden/make_grammar.py, every truncation of
// them and seeded byte flips through parse, init, the reject mask (decoded-once and per-step) and accept over a
// synthetic vocabulary, and checks only what must always hold: no crash, no sanitizer report, the two masks equal, the
// rejected count equal to the mask's bits, and an allowed token never leaving the grammar without a stack unless it
// decodes to U+0000.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ikoboldcpp_amd/csrc \
//       tools/grammar_fuzz.cpp -o /tmp/grammar_fuzz && /tmp/grammar_fuzz
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grammar.h"

static const char *const kGrammars[] = {
    "root ::= \"yes\" | \"no\" | \"maybe\" \"\\n\"",
    "root ::= (\"a\" (\"b\" | \"c\" (\"d\" | \"e\"))) \"!\"   # groups in groups\n",
    "root ::= \"a\"* \"b\"+ \"c\"? [0-9]{2} \"x\"{1,3} \"y\"{2,} \"\\n\"",
    "root ::= [a-cX-Z0-9_]+ [^a-z\\n] . [^\\x00-\\x7f]? \".\"\n",
    "root ::= \"\\t\\\"\\\\\" \"\\x41\\u00e9\\U0001F600\" [\\]\\[] \"\\n\"",
    "# a JSON-like grammar\n"
    "root   ::= value\n"
    "value  ::= object | array | string | number | \"true\" | \"false\" | \"null\"\n"
    "object ::= \"{\" ws ( pair ( \",\" ws pair )* )? \"}\"\n"
    "pair   ::= string ws \":\" ws value ws\n"
    "array  ::= \"[\" ws ( value ws ( \",\" ws value ws )* )? \"]\"\n"
    "string ::= \"\\\"\" ( [^\"\\\\\\x00-\\x1f] | \"\\\\\" ( [\"\\\\/bfnrt] | \"u\" [0-9a-fA-F]{4} ) )* \"\\\"\"\n"
    "number ::= \"-\"? ( \"0\" | [1-9] [0-9]* ) ( \".\" [0-9]+ )?\n"
    "ws     ::= [ \\t\\n]*\n",
    "root ::= (\"yes\" | \"no\") \" \" [0-9]{3}",
    "root ::= ws \"k\" ws \"k\"\nws ::= | \" \" ws\n",
    "root ::= \"h\xc3\xa9llo\" \" \" \"\xe6\x97\xa5\xe6\x9c\xac\" \"\xf0\x9f\x98\x80\"? [\xe3\x81\x80-\xe3\x83\xbf]*",
    "root ::= item+\r\nitem ::= \"- \" word \"\\n\"\r\nword ::= [a-z]+ | [0-9]+\r\n",
    "root ::= (\"a\" \"b\"",
    "root ::= \"a\" thing",
    "root ::= root \"a\" | \"b\"",
    "root ::= opt root \"a\" | \"b\"\nopt ::= \"x\" |",
    "root ::= opt root \"a\" | \"b\"\nopt ::= \"x\"?",        // the reference's detection misses this one and recurses without end
    "start ::= \"a\"",
    "root ::= \"a\"{99999999}",
    "root ::= (\"a\"?){3000}",
    "root ::= (((\"a\"?)?)?)* \"b\"",
    "root ::= a\na ::= b\nb ::= c\nc ::= d\nd ::= \"x\" | a? \"y\"",
    "root ::= \"a\"{2147483648,5}",                         // counts past an int, past the limit, and max below min
    "root ::= \"a\"{4294967295}",
    "root ::= \"a\"{18446744073709551615,}",
    "root ::= \"a\"{1048577}",
    "root ::= \"a\"{5,2} \"b\"",
    "root ::= s\ns ::= g s |\ng ::= h\nh ::= \"a\" |",           // expands without end behind a passed left-recursion check
};

static std::vector<std::string> make_vocab() {
    std::vector<std::string> v;
    for (int b = 1; b < 256; ++b) v.push_back(std::string(1, (char)b));
    const char *multi[] = {"ye", "s\n", "{\"", "yes", "no", " ", "true", "fal", "se", "null", "\":", "\", \"", "12", "007", "ab", "- a",
                           "h\xc3", "\xa9llo", "\xe6\x97", "\x97\xa5", "\xf0\x9f", "\x98\x80", "\xf0\x9f\x98", "\xc0\x80", "a\x80", "\xc3(",
                           "\xe3\x81\x82", "\xf8\x88"};
    for (const char *m : multi) v.push_back(m);
    v.push_back(std::string());
    v.push_back(std::string("\0a", 2));
    v.push_back(std::string());                // EOS
    return v;
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

static long g_loaded = 0, g_steps = 0;

static int run(const std::string &text, const std::vector<std::string> &vocab, const kgram::VocabCache &vc,
               const std::vector<const char *> &ptr, const std::vector<size_t> &len) {
    kgram::Grammar g;
    if (!kgram::load(g, text.c_str())) return 0;
    ++g_loaded;
    const int n = (int)vocab.size(), eos = n - 1;
    std::vector<uint32_t> m1((n + 31) / 32), m2((n + 31) / 32);
    kgram::MaskWork w;
    for (int step = 0; step < 24; ++step) {
        const int n1 = kgram::reject_mask(g, vc, ptr.data(), len.data(), n, eos, -1, false, w, m1.data());
        const int n2 = kgram::reject_mask(g, vc, ptr.data(), len.data(), n, eos, -1, true, w, m2.data());
        if (n1 == -2 || n2 == -2) return 0;                      // a limit: a status, the request ends
        int bits = 0;
        for (uint32_t x : m1) bits += __builtin_popcount(x);
        if (n1 != n2 || m1 != m2 || bits != n1) { fprintf(stderr, "mask mismatch: %s\n", text.c_str()); return 1; }
        std::vector<int> allowed;
        for (int i = 0; i < n; ++i)
            if (!kgram::mask_bit(m1.data(), i)) allowed.push_back(i);
        if (allowed.empty()) return 0;
        const int t = allowed[rnd() % allowed.size()];
        ++g_steps;
        const int rc = kgram::accept_piece(g, vocab[t].data(), vocab[t].size(), t == eos);
        if (t == eos) return rc ? (fprintf(stderr, "EOS allowed and refused: %s\n", text.c_str()), 1) : 0;
        if (rc == -2) {
            std::vector<uint32_t> cps;
            kgram::Partial end;
            kgram::decode_utf8(vocab[t].data(), vocab[t].size(), kgram::Partial{0, 0}, cps, &end);
            if (g.overflow || cps[0] == 0) return 0;             // a limit, or the overlong U+0000 the mask lets through
            fprintf(stderr, "allowed token %d left no stack: %s\n", t, text.c_str());
            return 1;
        }
    }
    return 0;
}

int main() {
    const std::vector<std::string> vocab = make_vocab();
    std::vector<const char *> ptr;
    std::vector<size_t> len;
    for (const std::string &p : vocab) ptr.push_back(p.data()), len.push_back(p.size());
    kgram::VocabCache vc;
    vc.build((int)vocab.size(), [&](int i) { return vocab[i]; });
    long n_run = 0;
    int bad = 0;
    for (const char *gt : kGrammars) {
        const std::string text = gt;
        bad += run(text, vocab, vc, ptr, len), ++n_run;
        for (size_t cut = 0; cut < text.size(); cut += 3) bad += run(text.substr(0, cut), vocab, vc, ptr, len), ++n_run;
        for (int k = 0; k < 40; ++k) {
            std::string t = text;
            const int flips = 1 + (int)(rnd() % 3);
            for (int f = 0; f < flips; ++f) {
                const size_t at = rnd() % t.size();
                const uint32_t how = rnd() % 4;
                if (how == 0) t[at] = (char)(t[at] ^ (1 << (rnd() % 8)));
                else if (how == 1) t[at] = "()[]{}|*+?\"\\^-.,#\n:= 09az"[rnd() % 25];
                else if (how == 2) t.insert(at, 1, "([{\"\\|"[rnd() % 6]);
                else t.erase(at, 1);
                if (t.empty()) t = "r";
            }
            for (char &c : t)
                if (c == 0) c = ' ';                             // the text is a C string
            bad += run(t, vocab, vc, ptr, len), ++n_run;
        }
    }
    printf("grammar_fuzz: %ld texts, %ld gave a grammar, %ld accepted tokens, %d failures\n", n_run, g_loaded, g_steps, bad);
    return bad ? 1 : 0;
}
