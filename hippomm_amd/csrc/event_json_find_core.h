// Where the `[[numbers], ...]` matrices of an event file lie, decided byte by byte: the pieces the gfx950 kernels of
// event_json_find.hip and their host twin (hmm_json_find_matrices_blocks) are both made of.  The oracle is hmm_json_find_matrices
// (event_json.cpp); its answer decomposes into rules that need no sequential walk:
//
//   1. STRING STATE.  Three states: outside a string, inside, inside behind a backslash.  A byte is a map of the three states
//      (`"` enters and leaves, `\` inside makes the next byte inert, everything else keeps the state); maps compose associatively,
//      so the state in front of any byte is a prefix "sum" of maps (6 bits each).
//   2. THE LAST NON-WHITESPACE BYTE.  Every byte outside strings is judged from its own class and the class of the previous byte
//      that is not whitespace -- where a comma remembers whether it stands behind a token or behind a `]`.  With that one refinement
//      the matrix grammar `[ [ T (, T)* ] (, [ T (, T)* ])* ]` is a chain of allowed pairs:
//          [ -> [    a CANDIDATE (the first of the two) and the first row       [ -> T    T -> ,t    ,t -> T    T -> ]
//          ] -> ,r   ,r -> [ (a row)                                            ] -> ]    a CLOSER
//      and every other pair, every quote and every byte inside a string is ILLEGAL for a matrix.  "The last non-whitespace class and
//      where it stood" is again an associative "last one wins" summary (a comma that is the first of its piece is resolved by the
//      piece in front).
//   3. A candidate is a matrix iff the next event (candidate or closer) behind it is a closer and no illegal byte lies between;
//      rows = row starts between, rows x cols = tokens between, both differences of prefix counts; the rows are equally long iff
//      the row start with relative ordinal k has relative token ordinal k * cols.
//   A token is a maximal run of bytes outside strings that are neither whitespace, `,`, `[`, `]` nor `"`; it is judged at its first
//   byte: JSON's number grammar with NaN / Infinity / -Infinity, exactly scan_number's (event_json.cpp).  A run of more than
//   HMM_JSON_TOKEN_MAX number bytes is not judged but counted (LONG): a candidate that is otherwise a matrix and holds one makes the
//   finder decline.
// Only closers whose previous event is a candidate can end a matrix, and only those are recorded, so the event list holds at most
// two entries per candidate.
#pragma once
#include <stdint.h>
#include "event_json_core.h"

#ifndef HMM_JSON_TOKEN_MAX
#define HMM_JSON_TOKEN_MAX 64                                  // include/hippomm_hip.h states the same
#endif

namespace hmm_find {

constexpr uint32_t kBytesPerThread = 16;
// how many of the 16 bytes from text offset at0 on lie inside a text of len bytes
HMM_JSON_HD uint32_t bytes_in_text(uint64_t len, uint64_t at0) {
    return at0 >= len ? 0u : (len - at0 < kBytesPerThread ? (uint32_t)(len - at0) : kBytesPerThread);
}

// ---- 1. string state ----
constexpr uint32_t kOut = 0, kIn = 1, kEsc = 2;
// bits [2 s + 1 : 2 s] of a map: the image of state s
constexpr uint32_t kMapIdentity = 0x24, kMapQuote = 0x11, kMapBackslash = 0x18, kMapOther = 0x14;

HMM_JSON_HD uint32_t map_apply(uint32_t m, uint32_t s) { return (m >> (2 * s)) & 3; }
// a, then b
HMM_JSON_HD uint32_t map_compose(uint32_t a, uint32_t b) {
    return map_apply(b, map_apply(a, 0)) | (map_apply(b, map_apply(a, 1)) << 2) | (map_apply(b, map_apply(a, 2)) << 4);
}
HMM_JSON_HD uint32_t byte_map(uint32_t c) { return c == '"' ? kMapQuote : c == '\\' ? kMapBackslash : kMapOther; }

HMM_JSON_HD bool is_ws(uint32_t c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r'; }
// what ends a token: whitespace, the structural bytes, and a quote
HMM_JSON_HD bool ends_token(uint32_t c) { return is_ws(c) || c == ',' || c == '[' || c == ']' || c == '"'; }
HMM_JSON_HD bool is_digit(uint32_t c) { return c >= '0' && c <= '9'; }
HMM_JSON_HD bool is_number_byte(uint32_t c) {
    return is_digit(c) || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E' || c == 'N' || c == 'a' || c == 'I' || c == 'n' || c == 'f' ||
           c == 'i' || c == 't' || c == 'y';
}

// ---- 2. the last non-whitespace byte ----
enum Last : uint32_t { kNone = 0, kOpen = 1, kClose = 2, kTok = 3, kQ = 4, kCommaT = 5, kCommaR = 6, kCommaX = 7, kCommaU = 8 };

// the class of a comma behind `prev`: kCommaU while the piece in front is not known
HMM_JSON_HD uint32_t comma_behind(uint32_t prev) { return prev == kTok ? kCommaT : prev == kClose ? kCommaR : prev == kNone ? kCommaU : kCommaX; }
// the class of piece b's last byte (cb) once the class in front of the piece (ca) is known
HMM_JSON_HD uint32_t last_class_behind(uint32_t ca, uint32_t cb) { return cb == kNone ? ca : cb == kCommaU ? comma_behind(ca) : cb; }
// packed for one group: class << 16 | byte offset in the group; 0: the piece has no such byte
HMM_JSON_HD uint32_t last_pack(uint32_t cls, uint32_t pos) { return (cls << 16) | pos; }
HMM_JSON_HD uint32_t last_compose(uint32_t a, uint32_t b) {
    const uint32_t cb = b >> 16;
    if (cb == kNone) return a;
    return (last_class_behind(a >> 16, cb) << 16) | (b & 0xFFFF);
}

// ---- 3. events of a piece: n recorded (bits 0..12), any event (13), the first is a closer whose recording depends on the piece in
// front (14; not counted in n), the last is a candidate (15), candidates (16..28) ----
constexpr uint32_t kEvHas = 1u << 13, kEvFirstCloser = 1u << 14, kEvLastCand = 1u << 15, kEvCandShift = 16, kEvCountMask = 0x1FFF;

HMM_JSON_HD uint32_t events_compose(uint32_t a, uint32_t b) {
    if (!(b & kEvHas)) return a;
    if (!(a & kEvHas)) return b;
    const uint32_t n = (a & kEvCountMask) + (b & kEvCountMask) + (((b & kEvFirstCloser) && (a & kEvLastCand)) ? 1u : 0u);
    const uint32_t cands = (a >> kEvCandShift) + (b >> kEvCandShift);
    return n | kEvHas | (a & kEvFirstCloser) | (b & kEvLastCand) | (cands << kEvCandShift);
}
// a thread's 16 bytes: bit i of cand / closer
HMM_JSON_HD uint32_t events_of(uint32_t cand, uint32_t closer) {
    uint32_t ev = cand | closer;
    if (!ev) return 0;
    uint32_t n = 0, out = kEvHas;
    bool last_cand = false, first = true;
    while (ev) {
        const uint32_t bit = ev & (0u - ev);
        ev ^= bit;
        const bool is_cand = (cand & bit) != 0;
        if (is_cand || last_cand) ++n;
        else if (first) out |= kEvFirstCloser;
        last_cand = is_cand;
        first = false;
    }
    uint32_t c = cand, cands = 0;
    while (c) { c &= c - 1; ++cands; }
    return out | n | (last_cand ? kEvLastCand : 0u) | (cands << kEvCandShift);
}

// ---- a token, judged at its first byte.  at(k): the byte k behind the thread's first; a space behind the end of the text ----
enum Judged : int { kNumber = 0, kBadToken = 1, kLongToken = 2 };

template <typename At>
HMM_JSON_HD bool number_grammar(const At& at, int p, int n) {
    int i = p;
    const int e = p + n;
    const bool neg = at(i) == '-';
    if (neg) ++i;
    if (e - i == 8) {
        const char* s = "Infinity";
        bool same = true;
        for (int j = 0; j < 8; ++j) same &= at(i + j) == (uint32_t)s[j];
        if (same) return true;
    }
    if (!neg && n == 3 && at(p) == 'N' && at(p + 1) == 'a' && at(p + 2) == 'N') return true;
    if (i >= e || !is_digit(at(i))) return false;
    if (at(i) == '0') ++i;
    else
        while (i < e && is_digit(at(i))) ++i;
    if (i < e && at(i) == '.') {
        ++i;
        if (i >= e || !is_digit(at(i))) return false;
        while (i < e && is_digit(at(i))) ++i;
    }
    if (i < e && (at(i) == 'e' || at(i) == 'E')) {
        ++i;
        if (i < e && (at(i) == '+' || at(i) == '-')) ++i;
        if (i >= e || !is_digit(at(i))) return false;
        while (i < e && is_digit(at(i))) ++i;
    }
    return i == e;
}

template <typename At>
HMM_JSON_HD int judge_token(const At& at, int p) {
    int len = 0;
    for (; len <= HMM_JSON_TOKEN_MAX; ++len) {
        const uint32_t c = at(p + len);
        if (ends_token(c)) break;
        if (!is_number_byte(c)) return kBadToken;
    }
    if (len > HMM_JSON_TOKEN_MAX) return kLongToken;
    return number_grammar(at, p, len) ? kNumber : kBadToken;
}

// ---- one thread's 16 bytes ----
struct Walk {
    uint32_t tok, row, bad, lng, cand, closer;   // bit i: byte i starts a token / a row, is illegal, starts a long token, is the second
                                                 // bracket of a candidate, is a closer
    uint32_t nonws;                              // bit i: byte i is not whitespace outside strings
    uint32_t last;                               // last_pack of the last such byte, offsets counted from the thread's first byte; 0: none
    uint32_t map;                                // the string map of the bytes
};

// count: how many of the 16 bytes lie inside the text; first: the thread's first byte is the text's first; state: the string state in
// front; prev: the class of the last non-whitespace byte in front (kNone: not known yet -- only `last` and `map` mean something
// then); judge: tokens are judged (else every token counts as a number).
template <typename At>
HMM_JSON_HD void walk(const At& at, uint32_t count, bool first, uint32_t state, uint32_t prev, bool judge, Walk* w) {
    uint32_t tok = 0, row = 0, bad = 0, lng = 0, cand = 0, closer = 0, nonws = 0, last = 0, map = kMapIdentity;
    uint32_t need = 0;                                         // token starts where a number may stand: judged behind the loop, so that
                                                               // the lanes of a wave judge their first, second, ... token together
    for (uint32_t i = 0; i < kBytesPerThread; ++i) {
        if (i >= count) break;
        const uint32_t c = at((int)i), bit = 1u << i;
        map = map_compose(map, byte_map(c));
        if (state != kOut) {                                   // inside a string, its closing quote included
            state = map_apply(byte_map(c), state);
            bad |= bit;
            prev = kQ;
        } else if (is_ws(c)) {
            continue;
        } else if (c == '"') {
            state = kIn;
            bad |= bit;
            prev = kQ;
        } else if (c == '[') {
            if (prev == kOpen) cand |= bit;
            if (prev == kOpen || prev == kCommaR) row |= bit;
            else bad |= bit;
            prev = kOpen;
        } else if (c == ']') {
            if (prev == kClose) closer |= bit;
            else if (prev != kTok) bad |= bit;
            prev = kClose;
        } else if (c == ',') {
            prev = comma_behind(prev);
            if (prev == kCommaX) bad |= bit;
        } else {
            if ((first && i == 0) || ends_token(at((int)i - 1))) {
                tok |= bit;
                if (prev != kOpen && prev != kCommaT) bad |= bit;
                else if (judge) need |= bit;
            }
            prev = kTok;
        }
        nonws |= bit;
        last = last_pack(prev, i);
    }
    while (need) {
        const uint32_t bit = need & (0u - need);
        need ^= bit;
        const int j = judge_token(at, __builtin_ctz(bit));
        if (j == kBadToken) bad |= bit;
        if (j == kLongToken) lng |= bit;
    }
    w->tok = tok; w->row = row; w->bad = bad; w->lng = lng; w->cand = cand; w->closer = closer;
    w->nonws = nonws; w->last = last; w->map = map;
}

// ---- pairing: the event list entry, and a candidate against the entry behind it ----
struct Event { uint64_t pos, kind, tokens, rows, bad, longs; };          // pos: a candidate's first bracket / the byte behind a closer
constexpr uint64_t kEventCand = 1, kEventCloser = 2;

struct Matrix { uint64_t begin, end, rows, cols, tokens0, rows0, ragged, pad; };

enum Paired : int { kNoMatrix = 0, kMatrix = 1, kDeclineLong = 2 };

HMM_JSON_HD int pair_events(const Event& a, const Event& b, uint64_t min_values, Matrix* m) {
    if (a.kind != kEventCand || b.kind != kEventCloser || b.bad != a.bad) return kNoMatrix;
    const uint64_t rows = b.rows - a.rows, tokens = b.tokens - a.tokens;
    if (rows == 0 || tokens % rows != 0 || tokens < min_values) return kNoMatrix;
    if (b.longs != a.longs) return kDeclineLong;
    m->begin = a.pos; m->end = b.pos; m->rows = rows; m->cols = tokens / rows;
    m->tokens0 = a.tokens; m->rows0 = a.rows; m->ragged = 0; m->pad = 0;
    return kMatrix;
}

// the row start with `rows` row starts and `tokens` token starts in front of it, inside m: does it stand where equal rows put it?
HMM_JSON_HD bool row_in_place(const Matrix& m, uint64_t rows, uint64_t tokens) { return tokens - m.tokens0 == (rows - m.rows0) * m.cols; }

}  // namespace hmm_find
