// Driver behind tests/golden/make_grammar.py: runs the reference's grammar code (its llama-grammar.cpp, included as one
// translation unit from the reference tree given on the compiler's include path) on the maker's grammars, vocabulary
// and token walks, and prints what tests/golden/grammar.npz records.  Built into a temporary directory by the maker;
// nothing compiled from it is kept.
//
// The per-step mask and the accept step below follow koboldcpp's sample_grammar and grammar_accept_token
// (gpttype_adapter.cpp) over the reference's own decode_utf8, llama_grammar_reject_candidates and llama_grammar_accept.
//
// Input (stdin), one job:
//   V <n> <eos>            then n lines: the piece in hex ("-" for the empty piece)
//   G <hex of the GBNF>    one line per grammar, each followed by
//   W <steps> <seed> <n_forced> <forced ids...>
// Output per grammar: "NOGRAMMAR", or
//   RULES <n_rules>, then per rule "R <len> <type> <value> ..."
//   STACKS <n>
//   per step: "MASK <hex words>" (before the token), "TOK <id>", "STATE <n_stacks> <partial value> <partial n_remain>"
//   END
#include "llama-grammar.cpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// the one function of the reference's other files that this path calls (the left-recursion notice); the rest stays
// unresolved at link
void llama_log_internal(ggml_log_level, const char *, ...) {}

static std::string unhex(const std::string &h) {
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

static std::vector<std::string> g_vocab;
static int g_eos = -1;

// sample_grammar: the ids that get -INFINITY
static std::vector<uint32_t> step_mask(const llama_grammar *grammar) {
    const size_t n = g_vocab.size();
    std::vector<uint32_t> mask((n + 31) / 32, 0u);
    bool allow_eos = false;
    for (const auto &stack : grammar->stacks)
        if (stack.empty()) { allow_eos = true; break; }
    std::vector<std::pair<std::vector<uint32_t>, llama_partial_utf8>> decoded;
    decoded.reserve(n);
    std::vector<llama_grammar_candidate> cands;
    for (size_t i = 0; i < n; ++i) {
        const std::string &piece = g_vocab[i];
        if ((int)i == g_eos) {
            if (!allow_eos) mask[i >> 5] |= 1u << (i & 31);
        } else if (piece.empty() || piece[0] == 0) {
            mask[i >> 5] |= 1u << (i & 31);
        } else {
            decoded.push_back(decode_utf8(piece.c_str(), grammar->partial_utf8));
            cands.push_back({i, decoded.back().first.data(), decoded.back().second});
        }
    }
    for (const auto &r : llama_grammar_reject_candidates(grammar->rules, grammar->stacks, cands))
        mask[r.index >> 5] |= 1u << (r.index & 31);
    return mask;
}

// grammar_accept_token
static void accept_token(llama_grammar *grammar, int token) {
    if (token == g_eos) return;
    const auto decoded = decode_utf8(g_vocab[token].c_str(), grammar->partial_utf8);
    const auto &cps = decoded.first;
    for (auto it = cps.begin(), end = cps.end() - 1; it != end; ++it) {
        auto prev = grammar->stacks;
        llama_grammar_accept(grammar->rules, prev, *it, grammar->stacks);
    }
    grammar->partial_utf8 = decoded.second;
}

int main() {
    std::string line;
    llama_grammar *grammar = nullptr;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "V") {
            size_t n;
            is >> n >> g_eos;
            g_vocab.clear();
            for (size_t i = 0; i < n; ++i) {
                std::getline(std::cin, line);
                g_vocab.push_back(unhex(line));
            }
        } else if (cmd == "G") {
            std::string hex;
            is >> hex;
            const std::string text = unhex(hex);
            if (grammar) { llama_grammar_free_impl(grammar); grammar = nullptr; }
            llama_grammar_parser parser;               // a fresh parser per grammar
            parser.parse(text.c_str());
            if (!parser.rules.empty() && parser.symbol_ids.count("root")) {
                std::vector<const llama_grammar_element *> rules(parser.c_rules());
                grammar = llama_grammar_init_impl(nullptr, rules.data(), rules.size(), parser.symbol_ids.at("root"));
            }
            if (!grammar) { printf("NOGRAMMAR\n"); continue; }
            printf("RULES %zu\n", grammar->rules.size());
            for (const auto &rule : grammar->rules) {
                printf("R %zu", rule.size());
                for (const auto &e : rule) printf(" %d %u", (int)e.type, e.value);
                printf("\n");
            }
            printf("STACKS %zu\n", grammar->stacks.size());
        } else if (cmd == "W") {
            int steps, n_forced;
            unsigned seed;
            is >> steps >> seed >> n_forced;
            std::vector<int> forced(n_forced);
            for (int &f : forced) is >> f;
            if (!grammar) continue;
            for (int s = 0; s < steps; ++s) {
                const std::vector<uint32_t> mask = step_mask(grammar);
                std::vector<int> allowed;
                for (size_t i = 0; i < g_vocab.size(); ++i)
                    if (!((mask[i >> 5] >> (i & 31)) & 1u)) allowed.push_back((int)i);
                printf("MASK");
                for (uint32_t w : mask) printf(" %08x", w);
                printf("\n");
                if (allowed.empty()) break;
                int tok;
                if (s < n_forced) {
                    tok = forced[s];
                    if ((mask[tok >> 5] >> (tok & 31)) & 1u) { printf("ERR forced token %d is rejected at step %d\n", tok, s); return 1; }
                } else {
                    // a seeded choice among the allowed tokens; one that would leave no stack (an overlong encoding of
                    // U+0000 passes the mask as an empty token) is passed over while another is to be had
                    seed = seed * 1664525u + 1013904223u;
                    const size_t first = (seed >> 8) % allowed.size();
                    tok = allowed[first];
                    for (size_t k = 0; k < allowed.size(); ++k) {
                        const int cand = allowed[(first + k) % allowed.size()];
                        const auto stacks = grammar->stacks;
                        const auto partial = grammar->partial_utf8;
                        accept_token(grammar, cand);
                        const bool alive = !grammar->stacks.empty();
                        grammar->stacks = stacks;
                        grammar->partial_utf8 = partial;
                        if (alive) { tok = cand; break; }
                    }
                }
                accept_token(grammar, tok);
                printf("TOK %d\n", tok);
                printf("STATE %zu %u %d\n", grammar->stacks.size(), grammar->partial_utf8.value, grammar->partial_utf8.n_remain);
                if (tok == g_eos || grammar->stacks.empty()) break;
            }
            printf("END\n");
        }
    }
    return 0;
}
