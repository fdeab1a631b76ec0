// grammar.h -- GBNF grammar-constrained sampling: the parser, the pushdown stack set, the per-step reject mask and the
// accept step.  Host-only plain C++ (no HIP), the idiom of sampler.h: a restatement of what the reference runs around
// SampleLogits when a request carries a grammar (load_grammar, sample_grammar, grammar_accept_token in
// gpttype_adapter.cpp over llama-grammar.cpp's parser and matcher), pinned to it by tests/test_grammar.py.
//
// A grammar is a list of rules; a rule is an array of (type, value) elements: alternates separated by ALT, closed by
// END; a character set is CHAR or CHAR_NOT followed by CHAR_ALT / CHAR_RNG_UPPER continuations; "." is CHAR_ANY;
// repetitions and groups become synthesized rules.  The state is a set of stacks of positions, each stack's top at a
// character element (an empty stack: the grammar may end here), plus the bytes of a UTF-8 character that a token left
// unfinished.  Per step every vocabulary piece is tested against the stack set: reject_mask() gives the bitmask of
// rejected ids that the sampling front end (cand.h) and the masked argmax take.
//
// Unlike the reference this code meets its input with bounds instead of aborts: nesting, rule count, element count,
// the depth of advance_stack and the size of the stack set are limited (the limits below); a grammar beyond them is
// "no grammar" at load, or a status (Grammar::overflow) afterwards.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace kgram {

enum { G_END = 0, G_ALT = 1, G_RULE_REF = 2, G_CHAR = 3, G_CHAR_NOT = 4, G_CHAR_RNG_UPPER = 5, G_CHAR_ALT = 6, G_CHAR_ANY = 7 };
struct Elem { uint32_t type, value; };
using Rule = std::vector<Elem>;
struct Partial { uint32_t value; int32_t n_remain; };    // an unfinished UTF-8 character: bits so far, bytes missing (-1: invalid)

constexpr int MAX_NEST = 128;            // nested groups in the text
constexpr size_t MAX_RULES = 1 << 16;
constexpr size_t MAX_ELEMS = 1 << 20;    // over all rules
constexpr int MAX_DEPTH = 1024;          // advance_stack / left-recursion recursion
constexpr size_t MAX_STACKS = 1 << 14;
constexpr size_t MAX_WORK = 1 << 22;     // advance_stack calls of one load, one mask or one accepted piece
constexpr int MAX_COUNT = 1 << 20;       // a repetition count in the text ({m}, {m,n}): MAX_ELEMS could not hold more

// ---- UTF-8 with a carried partial state (a piece is read up to its first zero byte, as a C string)
inline void decode_utf8(const char *src, size_t len, Partial start, std::vector<uint32_t> &cps, Partial *end) {
    static const int lookup[] = {1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 3, 4};
    size_t pos = 0;
    auto at = [&](size_t p) -> uint8_t { return p < len ? (uint8_t)src[p] : 0; };
    cps.clear();
    uint32_t value = start.value;
    int n_remain = start.n_remain;
    while (at(pos) != 0 && n_remain > 0) {               // continue the previous character
        const uint8_t b = at(pos);
        if ((b >> 6) != 2) {
            cps.push_back(0);
            *end = Partial{0, -1};
            return;
        }
        value = (value << 6) + (b & 0x3F);
        ++pos, --n_remain;
    }
    if (start.n_remain > 0 && n_remain == 0) cps.push_back(value);
    while (at(pos) != 0) {
        const uint8_t first = at(pos);
        n_remain = lookup[first >> 4] - 1;
        if (n_remain < 0) {                              // a continuation byte where a character starts
            cps.clear();
            cps.push_back(0);
            *end = Partial{0, n_remain};
            return;
        }
        value = first & ((1u << (7 - n_remain)) - 1);
        ++pos;
        while (at(pos) != 0 && n_remain > 0) {
            value = (value << 6) + (at(pos) & 0x3F);
            ++pos, --n_remain;
        }
        if (n_remain == 0) cps.push_back(value);
    }
    cps.push_back(0);
    *end = Partial{value, n_remain};
}

// ---- the GBNF parser
struct ParseError {};
struct Parser {
    std::map<std::string, uint32_t> symbol_ids;
    std::vector<Rule> rules;
    size_t n_elems = 0;
    int nest = 0;

    static bool is_digit(char c) { return '0' <= c && c <= '9'; }
    static bool is_word(char c) { return ('a' <= c && c <= 'z') || ('A' <= c && c <= 'Z') || c == '-' || is_digit(c); }
    uint32_t get_symbol_id(const char *src, size_t len) {
        const uint32_t next = (uint32_t)symbol_ids.size();
        return symbol_ids.emplace(std::string(src, len), next).first->second;
    }
    uint32_t generate_symbol_id(const std::string &base) {
        const uint32_t next = (uint32_t)symbol_ids.size();
        symbol_ids[base + '_' + std::to_string(next)] = next;
        return next;
    }
    void push(Rule &r, Elem e) {
        if (++n_elems > MAX_ELEMS) throw ParseError{};
        r.push_back(e);
    }
    void add_rule(uint32_t id, const Rule &r) {
        if (id >= MAX_RULES) throw ParseError{};
        if (rules.size() <= id) rules.resize(id + 1);
        rules[id] = r;
    }
    static const char *parse_space(const char *pos, bool newline_ok) {
        while (*pos == ' ' || *pos == '\t' || *pos == '#' || (newline_ok && (*pos == '\r' || *pos == '\n'))) {
            if (*pos == '#')
                while (*pos && *pos != '\r' && *pos != '\n') ++pos;
            else
                ++pos;
        }
        return pos;
    }
    static const char *parse_name(const char *src) {
        const char *pos = src;
        while (is_word(*pos)) ++pos;
        if (pos == src) throw ParseError{};
        return pos;
    }
    // digits; above MAX_COUNT: an error (the reference narrows std::stoul's value to an int and goes on with whatever
    // that gives, a negative count included)
    static int parse_count(const char *&pos) {
        if (!is_digit(*pos)) throw ParseError{};
        int v = 0;
        while (is_digit(*pos)) {
            v = v * 10 + (*pos - '0');
            if (v > MAX_COUNT) throw ParseError{};
            ++pos;
        }
        return v;
    }
    static const char *parse_hex(const char *src, int size, uint32_t *out) {
        const char *pos = src, *end = src + size;
        uint32_t value = 0;
        for (; pos < end && *pos; ++pos) {
            const char c = *pos;
            int d;
            if ('a' <= c && c <= 'f') d = c - 'a' + 10;
            else if ('A' <= c && c <= 'F') d = c - 'A' + 10;
            else if ('0' <= c && c <= '9') d = c - '0';
            else break;
            value = (value << 4) + (uint32_t)d;
        }
        if (pos != end) throw ParseError{};
        *out = value;
        return pos;
    }
    static const char *parse_char(const char *src, uint32_t *out) {
        if (*src == '\\') {
            switch (src[1]) {
                case 'x': return parse_hex(src + 2, 2, out);
                case 'u': return parse_hex(src + 2, 4, out);
                case 'U': return parse_hex(src + 2, 8, out);
                case 't': *out = '\t'; return src + 2;
                case 'r': *out = '\r'; return src + 2;
                case 'n': *out = '\n'; return src + 2;
                case '\\': case '"': case '[': case ']': *out = (uint32_t)src[1]; return src + 2;
                default: throw ParseError{};
            }
        }
        if (!*src) throw ParseError{};
        // one UTF-8 character by its lead byte's length, stopping at the text's end (a stray continuation byte counts as
        // a one-byte character)
        static const int lookup[] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4};
        const uint8_t first = (uint8_t)*src;
        const int len = lookup[first >> 4];
        uint32_t value = first & (uint8_t)((1 << (8 - len)) - 1);
        const char *pos = src + 1;
        for (int i = 1; i < len && *pos; ++i, ++pos) value = (value << 6) + ((uint8_t)*pos & 0x3F);
        *out = value;
        return pos;
    }
    // the previous symbol (rule[last_sym_start ...]) repeated min..max times (max < 0: no upper end):
    //   S{m,n} -> S x m, then S'(n-m) with S'(x) ::= S S'(x-1) | and S'(1) ::= S |
    //   S{m,}  -> S x m, then S' with S' ::= S S' |
    void repetitions(Rule &rule, size_t last_sym_start, const std::string &rule_name, int min_times, int max_times) {
        if (last_sym_start == rule.size()) throw ParseError{};
        const Rule prev(rule.begin() + last_sym_start, rule.end());
        if (min_times == 0) {
            n_elems -= rule.size() - last_sym_start;
            rule.resize(last_sym_start);
        } else {
            for (int i = 1; i < min_times; ++i)
                for (const Elem &e : prev) push(rule, e);
        }
        uint32_t last_rec = 0;
        const int n_opt = max_times < 0 ? 1 : max_times - min_times;    // both <= MAX_COUNT; max < min: as if max were min
        Rule rec(prev);
        for (int i = 0; i < n_opt; ++i) {
            rec.resize(prev.size());
            const uint32_t rec_id = generate_symbol_id(rule_name);
            if (i > 0 || max_times < 0) rec.push_back(Elem{G_RULE_REF, max_times < 0 ? rec_id : last_rec});
            rec.push_back(Elem{G_ALT, 0});
            rec.push_back(Elem{G_END, 0});
            if ((n_elems += rec.size()) > MAX_ELEMS) throw ParseError{};
            add_rule(rec_id, rec);
            last_rec = rec_id;
        }
        if (n_opt > 0) push(rule, Elem{G_RULE_REF, last_rec});
    }
    const char *parse_sequence(const char *src, const std::string &rule_name, Rule &rule, bool nested) {
        size_t last_sym_start = rule.size();
        const char *pos = src;
        while (*pos) {
            if (*pos == '"') {
                ++pos;
                last_sym_start = rule.size();
                while (*pos != '"') {
                    if (!*pos) throw ParseError{};
                    uint32_t c;
                    pos = parse_char(pos, &c);
                    push(rule, Elem{G_CHAR, c});
                }
                pos = parse_space(pos + 1, nested);
            } else if (*pos == '[') {
                ++pos;
                uint32_t start_type = G_CHAR;
                if (*pos == '^') { ++pos; start_type = G_CHAR_NOT; }
                last_sym_start = rule.size();
                while (*pos != ']') {
                    if (!*pos) throw ParseError{};
                    uint32_t c;
                    pos = parse_char(pos, &c);
                    push(rule, Elem{last_sym_start < rule.size() ? (uint32_t)G_CHAR_ALT : start_type, c});
                    if (pos[0] == '-' && pos[1] != ']') {
                        if (!pos[1]) throw ParseError{};
                        pos = parse_char(pos + 1, &c);
                        push(rule, Elem{G_CHAR_RNG_UPPER, c});
                    }
                }
                pos = parse_space(pos + 1, nested);
            } else if (is_word(*pos)) {
                const char *name_end = parse_name(pos);
                const uint32_t ref = get_symbol_id(pos, (size_t)(name_end - pos));
                pos = parse_space(name_end, nested);
                last_sym_start = rule.size();
                push(rule, Elem{G_RULE_REF, ref});
            } else if (*pos == '(') {
                if (++nest > MAX_NEST) throw ParseError{};
                pos = parse_space(pos + 1, true);
                const uint32_t sub = generate_symbol_id(rule_name);
                pos = parse_alternates(pos, rule_name, sub, true);
                last_sym_start = rule.size();
                push(rule, Elem{G_RULE_REF, sub});
                if (*pos != ')') throw ParseError{};
                pos = parse_space(pos + 1, nested);
                --nest;
            } else if (*pos == '.') {
                last_sym_start = rule.size();
                push(rule, Elem{G_CHAR_ANY, 0});
                pos = parse_space(pos + 1, nested);
            } else if (*pos == '*') {
                pos = parse_space(pos + 1, nested);
                repetitions(rule, last_sym_start, rule_name, 0, -1);
            } else if (*pos == '+') {
                pos = parse_space(pos + 1, nested);
                repetitions(rule, last_sym_start, rule_name, 1, -1);
            } else if (*pos == '?') {
                pos = parse_space(pos + 1, nested);
                repetitions(rule, last_sym_start, rule_name, 0, 1);
            } else if (*pos == '{') {
                pos = parse_space(pos + 1, nested);
                const int min_times = parse_count(pos);
                pos = parse_space(pos, nested);
                int max_times = -1;
                if (*pos == '}') {
                    max_times = min_times;
                    pos = parse_space(pos + 1, nested);
                } else if (*pos == ',') {
                    pos = parse_space(pos + 1, nested);
                    if (is_digit(*pos)) {
                        max_times = parse_count(pos);
                        pos = parse_space(pos, nested);
                    }
                    if (*pos != '}') throw ParseError{};
                    pos = parse_space(pos + 1, nested);
                } else {
                    throw ParseError{};
                }
                repetitions(rule, last_sym_start, rule_name, min_times, max_times);
            } else {
                break;
            }
        }
        return pos;
    }
    const char *parse_alternates(const char *src, const std::string &rule_name, uint32_t rule_id, bool nested) {
        Rule rule;
        const char *pos = parse_sequence(src, rule_name, rule, nested);
        while (*pos == '|') {
            push(rule, Elem{G_ALT, 0});
            pos = parse_space(pos + 1, true);
            pos = parse_sequence(pos, rule_name, rule, nested);
        }
        push(rule, Elem{G_END, 0});
        add_rule(rule_id, rule);
        return pos;
    }
    const char *parse_rule(const char *src) {
        const char *name_end = parse_name(src);
        const char *pos = parse_space(name_end, false);
        const size_t name_len = (size_t)(name_end - src);
        const uint32_t rule_id = get_symbol_id(src, name_len);
        const std::string name(src, name_len);
        if (!(pos[0] == ':' && pos[1] == ':' && pos[2] == '=')) throw ParseError{};
        pos = parse_space(pos + 3, true);
        pos = parse_alternates(pos, name, rule_id, false);
        if (*pos == '\r') pos += pos[1] == '\n' ? 2 : 1;
        else if (*pos == '\n') ++pos;
        else if (*pos) throw ParseError{};
        return parse_space(pos, true);
    }
    // any error (syntax, a rule referenced and never defined, a limit): no rules, false
    bool parse(const char *src) {
        try {
            const char *pos = parse_space(src, true);
            while (*pos) pos = parse_rule(pos);
            for (const Rule &r : rules) {
                if (r.empty()) throw ParseError{};
                for (const Elem &e : r)
                    if (e.type == G_RULE_REF && (e.value >= rules.size() || rules[e.value].empty())) throw ParseError{};
            }
        } catch (const ParseError &) {
            rules.clear();
            return false;
        } catch (const std::exception &) {       // allocation
            rules.clear();
            return false;
        }
        return true;
    }
};

// ---- the matcher
using Stack = std::vector<const Elem *>;
using Stacks = std::vector<Stack>;
struct Cand { uint32_t index; const uint32_t *cp; Partial partial; };

inline bool is_end_of_sequence(const Elem *pos) { return pos->type == G_END || pos->type == G_ALT; }

// does chr satisfy the character set at pos; *after: the element behind the set
inline bool match_char(const Elem *pos, uint32_t chr, const Elem **after) {
    bool found = false;
    const bool positive = pos->type == G_CHAR || pos->type == G_CHAR_ANY;
    do {
        if (pos[1].type == G_CHAR_RNG_UPPER) {
            found = found || (pos->value <= chr && chr <= pos[1].value);
            pos += 2;
        } else if (pos->type == G_CHAR_ANY) {
            found = true;
            pos += 1;
        } else {
            found = found || pos->value == chr;
            pos += 1;
        }
    } while (pos->type == G_CHAR_ALT);
    *after = pos;
    return found == positive;
}
// could some completion of the unfinished character satisfy the set at pos
inline bool match_partial_char(const Elem *pos, Partial pu) {
    const bool positive = pos->type == G_CHAR || pos->type == G_CHAR_ANY;
    const int n_remain = pu.n_remain;
    if (n_remain < 0 || (n_remain == 1 && pu.value < 2)) return false;      // invalid, or an overlong 7-bit character
    if (n_remain > 3) return false;                                         // no UTF-8 lead byte leaves more
    uint32_t low = pu.value << (n_remain * 6);
    const uint32_t high = low | ((1u << (n_remain * 6)) - 1);
    if (low == 0) {
        if (n_remain == 2) low = 1 << 11;
        else if (n_remain == 3) low = 1 << 16;
    }
    do {
        if (pos[1].type == G_CHAR_RNG_UPPER) {
            if (pos->value <= high && low <= pos[1].value) return positive;
            pos += 2;
        } else if (pos->type == G_CHAR_ANY) {
            return true;
        } else {
            if (low <= pos->value && pos->value <= high) return positive;
            pos += 1;
        }
    } while (pos->type == G_CHAR_ALT);
    return !positive;
}

struct Grammar {
    std::vector<Rule> rules;                 // never resized once stacks point into them
    Stacks stacks;
    Partial partial{0, 0};
    std::string source;                      // the text this state belongs to (grammar_retain_state)
    bool overflow = false;                   // a limit was hit while matching: the state is no longer the grammar's
    Grammar() = default;
    Grammar(const Grammar &) = delete;
    Grammar &operator=(const Grammar &) = delete;
    bool active() const { return !rules.empty(); }
    void clear() { stacks.clear(), rules.clear(), partial = Partial{0, 0}, overflow = false; }
};

// What bounds one piece of matching work (a load, a mask, an accepted piece).  Once overflow is set every function
// below returns at once, at entry and after each call it makes: the walk does not go on exploring, so a text whose
// expansion never ends (S ::= G S | with a G that is empty only through other rules passes the left-recursion check
// and re-enters S on both alternates at every level) costs MAX_DEPTH frames, not 2^MAX_DEPTH.
struct Guard { bool overflow = false; size_t work = 0; };

// a stack into the stacks it stands for, every one with a character element on top (or empty)
inline void advance_stack(const std::vector<Rule> &rules, const Stack &stack, Stacks &out, int depth, Guard *gd) {
    if (gd->overflow) return;
    auto add = [&](const Stack &s) {
        if (std::find(out.begin(), out.end(), s) != out.end()) return;
        if (out.size() >= MAX_STACKS) { gd->overflow = true; return; }
        out.push_back(s);
    };
    if (stack.empty()) { add(stack); return; }
    if (depth > MAX_DEPTH || ++gd->work > MAX_WORK) { gd->overflow = true; return; }
    const Elem *pos = stack.back();
    switch (pos->type) {
        case G_RULE_REF: {
            const Elem *sub = rules[pos->value].data();
            while (true) {
                Stack ns(stack.begin(), stack.end() - 1);
                if (!is_end_of_sequence(pos + 1)) ns.push_back(pos + 1);
                if (!is_end_of_sequence(sub)) ns.push_back(sub);
                advance_stack(rules, ns, out, depth + 1, gd);
                if (gd->overflow) return;
                while (!is_end_of_sequence(sub)) ++sub;
                if (sub->type != G_ALT) break;
                ++sub;
            }
            break;
        }
        case G_CHAR: case G_CHAR_NOT: case G_CHAR_ANY:
            add(stack);
            break;
        default:                             // a parsed rule never leaves a stack on END / ALT / a set's continuation
            gd->overflow = true;
    }
}

inline bool detect_left_recursion(const std::vector<Rule> &rules, size_t ri, std::vector<uint8_t> &visited,
                                  std::vector<uint8_t> &in_progress, std::vector<uint8_t> &may_be_empty, int depth) {
    if (in_progress[ri]) return true;
    if (depth > MAX_DEPTH) return true;      // deeper than the matcher may recurse: refused like left recursion
    in_progress[ri] = 1;
    const Rule &rule = rules[ri];
    bool at_start = true;
    for (size_t i = 0; i < rule.size(); ++i) {
        if (is_end_of_sequence(&rule[i])) {
            if (at_start) { may_be_empty[ri] = 1; break; }
            at_start = true;
        } else {
            at_start = false;
        }
    }
    bool recurse = true;
    for (size_t i = 0; i < rule.size(); ++i) {
        if (rule[i].type == G_RULE_REF && recurse) {
            if (detect_left_recursion(rules, rule[i].value, visited, in_progress, may_be_empty, depth + 1)) return true;
            if (!may_be_empty[rule[i].value]) recurse = false;
        } else if (is_end_of_sequence(&rule[i])) {
            recurse = true;
        } else {
            recurse = false;
        }
    }
    in_progress[ri] = 0;
    visited[ri] = 1;
    return false;
}

// load_grammar: parse, refuse left recursion, build the stacks of rule "root".  false: no grammar (g is cleared; the
// request runs unconstrained).  g.source is the caller's to set.
inline bool load(Grammar &g, const char *text) {
    g.clear();
    if (!text || !text[0]) return false;
    Parser p;
    if (!p.parse(text) || p.rules.empty()) return false;
    const auto root = p.symbol_ids.find("root");
    if (root == p.symbol_ids.end() || root->second >= p.rules.size()) return false;
    const size_t n = p.rules.size();
    std::vector<uint8_t> visited(n), in_progress(n), may_be_empty(n);
    for (size_t i = 0; i < n; ++i)
        if (!visited[i] && detect_left_recursion(p.rules, i, visited, in_progress, may_be_empty, 0)) return false;
    g.rules = std::move(p.rules);
    const Elem *pos = g.rules[root->second].data();
    Guard gd;
    while (!gd.overflow) {
        Stack s;
        if (!is_end_of_sequence(pos)) s.push_back(pos);
        advance_stack(g.rules, s, g.stacks, 0, &gd);
        while (!is_end_of_sequence(pos)) ++pos;
        if (pos->type != G_ALT) break;
        ++pos;
    }
    if (gd.overflow || g.stacks.empty()) { g.clear(); return false; }
    return true;
}

inline void reject_candidates(const std::vector<Rule> &rules, const Stacks &stacks, const std::vector<Cand> &cands,
                              std::vector<Cand> &rejects, Guard *gd);
inline void reject_for_stack(const std::vector<Rule> &rules, const Stack &stack, const std::vector<Cand> &cands,
                             std::vector<Cand> &rejects, Guard *gd) {
    rejects.clear();
    if (gd->overflow) return;
    if (stack.empty()) {
        for (const Cand &t : cands)
            if (*t.cp != 0 || t.partial.n_remain != 0) rejects.push_back(t);
        return;
    }
    const Elem *top = stack.back();
    std::vector<Cand> next;
    const Elem *after;
    for (const Cand &t : cands) {
        if (*t.cp == 0) {
            // the whole characters are through: rejected only for an unfinished one that cannot fit here
            if (t.partial.n_remain != 0 && !match_partial_char(top, t.partial)) rejects.push_back(t);
        } else if (match_char(top, *t.cp, &after)) {
            next.push_back(Cand{t.index, t.cp + 1, t.partial});
        } else {
            rejects.push_back(t);
        }
    }
    if (next.empty()) return;                // nothing to test deeper (the reference builds the stacks and finds the same)
    match_char(top, 0, &after);
    Stack stack_after(stack.begin(), stack.end() - 1);
    if (!is_end_of_sequence(after)) stack_after.push_back(after);
    Stacks next_stacks;
    advance_stack(rules, stack_after, next_stacks, 0, gd);
    if (gd->overflow) return;
    std::vector<Cand> next_rejects;
    reject_candidates(rules, next_stacks, next, next_rejects, gd);
    if (gd->overflow) return;
    for (const Cand &t : next_rejects) rejects.push_back(Cand{t.index, t.cp - 1, t.partial});
}
// the candidates that no stack accepts (with gd->overflow set on return: rejects says nothing)
inline void reject_candidates(const std::vector<Rule> &rules, const Stacks &stacks, const std::vector<Cand> &cands,
                              std::vector<Cand> &rejects, Guard *gd) {
    rejects.clear();
    if (cands.empty() || gd->overflow) return;
    if (stacks.empty()) { rejects = cands; return; }     // only after an overflow: nothing is accepted
    reject_for_stack(rules, stacks.front(), cands, rejects, gd);
    std::vector<Cand> tmp;
    for (size_t i = 1; i < stacks.size() && !rejects.empty() && !gd->overflow; ++i) {
        reject_for_stack(rules, stacks[i], rejects, tmp, gd);
        rejects.swap(tmp);
    }
}

// one code point accepted by every stack that can take it
inline void accept(Grammar &g, uint32_t chr, Guard *gd) {
    Stacks prev;
    prev.swap(g.stacks);
    const Elem *after;
    for (const Stack &s : prev) {
        if (s.empty()) continue;
        if (!match_char(s.back(), chr, &after)) continue;
        Stack ns(s.begin(), s.end() - 1);
        if (!is_end_of_sequence(after)) ns.push_back(after);
        advance_stack(g.rules, ns, g.stacks, 0, gd);
        if (gd->overflow) { g.overflow = true; return; }
    }
}
inline bool allows_end(const Grammar &g) {
    for (const Stack &s : g.stacks)
        if (s.empty()) return true;
    return false;
}

// grammar_accept_token.  0; -1: EOS / EOT while no stack is empty (the reference asserts); -2: no stack took the piece
// (the reference asserts) or a limit was hit.  The state after a negative return is not to be used.
inline int accept_piece(Grammar &g, const char *piece, size_t len, bool is_eos) {
    if (is_eos) return allows_end(g) ? 0 : -1;
    std::vector<uint32_t> cps;
    Partial end;
    decode_utf8(piece, len, g.partial, cps, &end);
    Guard gd;
    for (size_t i = 0; i + 1 < cps.size() && !gd.overflow; ++i) accept(g, cps[i], &gd);
    g.partial = end;
    return g.stacks.empty() || g.overflow ? -2 : 0;
}

// the vocabulary's pieces decoded once (from no carried state): what sample_grammar decodes again at every step
struct VocabCache {
    std::vector<uint32_t> cps;               // every piece's code points, each run closed by a 0
    std::vector<uint32_t> off;               // piece i starts at cps[off[i]]
    std::vector<Partial> end;
    std::vector<uint8_t> skip;               // an empty piece or one that starts with a zero byte: always rejected
    int n() const { return (int)skip.size(); }
    template <typename PieceFn>              // PieceFn(int id) -> std::string
    void build(int n_vocab, PieceFn piece) {
        cps.clear(), off.assign(n_vocab, 0), end.assign(n_vocab, Partial{0, 0}), skip.assign(n_vocab, 0);
        std::vector<uint32_t> one;
        for (int i = 0; i < n_vocab; ++i) {
            const std::string p = piece(i);
            off[i] = (uint32_t)cps.size();
            if (p.empty() || p[0] == 0) { skip[i] = 1; cps.push_back(0); continue; }
            decode_utf8(p.data(), p.size(), Partial{0, 0}, one, &end[i]);
            cps.insert(cps.end(), one.begin(), one.end());
        }
    }
};

// sample_grammar as a bitmask: bit i of mask[i / 32] set when token i is rejected -- EOS / EOT unless some stack is
// empty, empty pieces, and what reject_candidates returns.  use_cache: take the decoded pieces from vc when no
// character is carried over (the same code points; the tests hold the two equal); otherwise decode with the carried
// state.  Returns the number of rejected tokens, -2 when a limit was hit.
struct MaskWork { std::vector<Cand> cands, rejects; std::vector<uint32_t> cps, one; std::vector<size_t> at; };
inline int reject_mask(Grammar &g, const VocabCache &vc, const char *const *pieces, const size_t *lens, int n_vocab, int eos,
                       int eot, bool use_cache, MaskWork &w, uint32_t *mask) {
    const size_t nw = ((size_t)n_vocab + 31) / 32;
    std::fill(mask, mask + nw, 0u);
    const bool allow_eos = allows_end(g);
    const bool cached = use_cache && g.partial.n_remain == 0 && vc.n() == n_vocab;
    w.cands.clear(), w.cps.clear(), w.at.clear();
    auto set = [&](uint32_t i) { mask[i >> 5] |= 1u << (i & 31); };
    for (int i = 0; i < n_vocab; ++i) {
        if (i == eos || (i == eot && i != -1)) {
            if (!allow_eos) set((uint32_t)i);
        } else if (cached ? vc.skip[i] != 0 : (lens[i] == 0 || pieces[i][0] == 0)) {
            set((uint32_t)i);
        } else if (cached) {
            w.cands.push_back(Cand{(uint32_t)i, vc.cps.data() + vc.off[i], vc.end[i]});
        } else {
            Partial end;
            decode_utf8(pieces[i], lens[i], g.partial, w.one, &end);
            w.at.push_back(w.cps.size());
            w.cps.insert(w.cps.end(), w.one.begin(), w.one.end());
            w.cands.push_back(Cand{(uint32_t)i, nullptr, end});
        }
    }
    if (!cached)
        for (size_t c = 0; c < w.cands.size(); ++c) w.cands[c].cp = w.cps.data() + w.at[c];
    Guard gd;
    reject_candidates(g.rules, g.stacks, w.cands, w.rejects, &gd);
    if (gd.overflow) { g.overflow = true; return -2; }
    for (const Cand &t : w.rejects) set(t.index);
    int n_rej = 0;
    for (size_t i = 0; i < nw; ++i) n_rej += __builtin_popcount(mask[i]);
    return n_rej;
}
inline bool mask_bit(const uint32_t *mask, int i) { return (mask[i >> 5] >> (i & 31)) & 1u; }

}  // namespace kgram
