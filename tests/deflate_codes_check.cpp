// deflate_codes_check.cpp -- csrc/deflate_codes.h as a stand-alone host program (tests/test_png_reference.py builds it with the
// address and undefined-behaviour sanitizers and runs it).
//
// For every histogram below: the code lengths lie within the limit; the Kraft sum is exactly 1 for two and more used symbols; the cost
// equals the Huffman cost whenever the Huffman tree (ties: the shallower subtree first, which makes the shallowest of the optimal
// trees) is no deeper than the limit, and is never below it.  Then whole blocks for token lists with these histograms are written
// through dc::write_block into the directory given as argv[1]: NAME.deflate, and NAME.expect with the bytes the block decodes to
// behind the preset dictionary dict(i) = (i * 7 + i / 251) & 255 of 32768 bytes; the Python test inflates them with zlib.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <string>
#include <vector>

#include "deflate_codes.h"

using namespace pamd;

static int g_checked = 0;

#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// The Huffman tree by a priority queue: (cost, depth of the deepest leaf).  Ties: the lighter first, then the shallower.
static void huffman(const std::vector<uint32_t> &freq, uint64_t &cost, unsigned &depth) {
    struct Node { uint64_t w; unsigned depth; };
    auto later = [](const Node &a, const Node &b) { return a.w != b.w ? a.w > b.w : a.depth > b.depth; };
    std::priority_queue<Node, std::vector<Node>, decltype(later)> q(later);
    for (uint32_t f : freq) if (f) q.push(Node{f, 0});
    cost = 0; depth = 0;
    if (q.size() == 1) { cost = q.top().w; depth = 1; return; }
    while (q.size() > 1) {
        const Node a = q.top(); q.pop();
        const Node b = q.top(); q.pop();
        cost += a.w + b.w;
        q.push(Node{a.w + b.w, std::max(a.depth, b.depth) + 1});
    }
    if (!q.empty()) depth = q.top().depth;
}

static void check_lengths(const char *name, const std::vector<uint32_t> &freq, unsigned limit) {
    const unsigned n = (unsigned)freq.size();
    std::vector<uint8_t> lens(n, 0xEE);
    std::vector<uint16_t> codes(n, 0xEEEE);
    dc::Work w;
    dc::code_lengths(freq.data(), n, limit, lens.data(), w, 0, 1, dc::NoSync{});
    unsigned used = 0;
    uint64_t kraft = 0, cost = 0;
    for (unsigned s = 0; s < n; s++) {
        if (!freq[s]) { CHECK(lens[s] == 0, "%s: unused symbol %u has length %u", name, s, lens[s]); continue; }
        used++;
        CHECK(lens[s] >= 1 && lens[s] <= limit, "%s: symbol %u has length %u, limit %u", name, s, lens[s], limit);
        kraft += (uint64_t)1 << (limit - lens[s]);
        cost += (uint64_t)freq[s] * lens[s];
    }
    if (used >= 2) CHECK(kraft == (uint64_t)1 << limit, "%s: Kraft sum %llu / %llu", name, (unsigned long long)kraft, 1ull << limit);
    if (used == 1) CHECK(cost == *std::max_element(freq.begin(), freq.end()), "%s: one symbol, length not 1", name);
    uint64_t best; unsigned depth;
    huffman(freq, best, depth);
    CHECK(cost >= best, "%s: cost %llu below Huffman's %llu", name, (unsigned long long)cost, (unsigned long long)best);
    if (depth <= limit) CHECK(cost == best, "%s: cost %llu, Huffman's %llu at depth %u", name, (unsigned long long)cost, (unsigned long long)best, depth);
    // heavier symbols never get longer codes
    for (unsigned a = 0; a < n; a++)
        for (unsigned b = 0; b < n; b++)
            if (freq[a] && freq[b] && freq[a] > freq[b]) CHECK(lens[a] <= lens[b], "%s: %u heavier than %u but longer", name, a, b);
    // canonical codes: prefix-free, read LSB first
    dc::canonical_codes(lens.data(), n, codes.data(), w, 0, 1, dc::NoSync{});
    for (unsigned a = 0; a < n; a++)
        for (unsigned b = a + 1; b < n; b++) {
            if (!lens[a] || !lens[b]) continue;
            const unsigned l = std::min(lens[a], lens[b]), mask = (1u << l) - 1u;
            CHECK((codes[a] & mask) != (codes[b] & mask), "%s: codes of %u and %u share a prefix", name, a, b);
        }
    g_checked++;
}

static unsigned char dict_byte(size_t i) { return (unsigned char)((i * 7 + i / 251) & 255); }

// the first length of a length symbol and the first distance of a distance symbol
static unsigned first_length(unsigned sym) { for (unsigned l = 3; l <= 258; l++) if (dc::length_symbol(l).sym == sym) return l; return 0; }
static unsigned last_length(unsigned sym) { for (unsigned l = 258; l >= 3; l--) if (dc::length_symbol(l).sym == sym) return l; return 0; }
static unsigned first_dist(unsigned sym) { for (unsigned d = 1; d <= 32768; d++) if (dc::dist_symbol(d).sym == sym) return d; return 0; }
static unsigned last_dist(unsigned sym) { for (unsigned d = 32768; d >= 1; d--) if (dc::dist_symbol(d).sym == sym) return d; return 0; }

// A block whose tokens have exactly the literal/length histogram `lit` (its end of block counts once) and use the distance symbols of
// `dist` in turn (none: the lengths are left out)
static void write_case(const std::string &dir, const char *name, const std::vector<uint32_t> &lit, const std::vector<uint32_t> &dist, bool final_block) {
    std::vector<uint32_t> tokens;
    std::vector<unsigned> dsyms;
    for (unsigned s = 0; s < dist.size(); s++) if (dist[s]) dsyms.push_back(s);
    size_t turn = 0;
    for (unsigned s = 0; s < lit.size(); s++)
        for (uint32_t c = 0; c < lit[s]; c++) {
            if (s < 256) tokens.push_back(s);
            else if (s > 256 && !dsyms.empty()) {
                const unsigned d = dsyms[turn % dsyms.size()];
                tokens.push_back(dc::tok_match(turn & 1 ? last_length(s) : first_length(s), turn & 2 ? last_dist(d) : first_dist(d)));
                turn++;
            }
        }
    // interleave: a fixed shuffle, so that matches and literals mix
    for (size_t i = 0; i + 1 < tokens.size(); i++) std::swap(tokens[i], tokens[i + (i * 2654435761u) % (tokens.size() - i)]);
    std::vector<unsigned char> text(32768);
    for (size_t i = 0; i < text.size(); i++) text[i] = dict_byte(i);
    for (uint32_t t : tokens) {
        if (!dc::tok_is_match(t)) { text.push_back((unsigned char)t); continue; }
        const unsigned len = dc::tok_len(t), d = dc::tok_dist(t);
        CHECK(len >= 3 && len <= 258 && d >= 1 && d <= 32768, "%s: token out of range", name);
        CHECK(dc::tok_is_match(t) && dc::length_symbol(len).sym >= 257 && dc::dist_symbol(d).sym < 30, "%s: symbol out of range", name);
        for (unsigned k = 0; k < len; k++) text.push_back(text[text.size() - d]);
    }
    dc::BitWriter bw;
    const uint64_t bits = dc::write_block(tokens.data(), tokens.size(), final_block, bw);
    CHECK(bits == bw.nbits && bw.bytes.size() == (bits + 7) / 8, "%s: bit count", name);
    CHECK(bits <= dc::block_bound_bits(text.size() - 32768), "%s: %llu bits beyond the bound of %zu bytes", name, (unsigned long long)bits, text.size() - 32768);
    if (!final_block) {                                                 // an empty final fixed block closes the stream
        bw.put(1, 1); bw.put(1, 2); bw.put(0, 7);
    }
    FILE *f = std::fopen((dir + "/" + name + ".deflate").c_str(), "wb");
    CHECK(f, "%s: cannot write", name);
    std::fwrite(bw.bytes.data(), 1, bw.bytes.size(), f);
    std::fclose(f);
    f = std::fopen((dir + "/" + name + ".expect").c_str(), "wb");
    CHECK(f, "%s: cannot write", name);
    std::fwrite(text.data() + 32768, 1, text.size() - 32768, f);
    std::fclose(f);
    std::printf("block %s: %zu tokens, %zu bytes in %llu bits\n", name, tokens.size(), text.size() - 32768, (unsigned long long)bits);
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    std::vector<uint32_t> lit(286, 0), dist(30, 0), none(30, 0);

    // the symbols and extra bits of every length and distance, against RFC 1951's tables
    static const unsigned len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const unsigned len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const unsigned dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    for (unsigned l = 3; l <= 258; l++) {
        unsigned s = 28;
        while (len_base[s] > l) s--;
        const dc::SymBits b = dc::length_symbol(l);
        CHECK(b.sym == 257 + s && b.nbits == len_extra[s] && b.bits == l - len_base[s] && dc::lit_extra_bits(b.sym) == b.nbits, "length %u", l);
    }
    for (unsigned d = 1; d <= 32768; d++) {
        unsigned s = 29;
        while (dist_base[s] > d) s--;
        const dc::SymBits b = dc::dist_symbol(d);
        CHECK(b.sym == s && b.nbits == (s < 4 ? 0 : s / 2 - 1) && b.bits == d - dist_base[s] && dc::dist_extra_bits(s) == b.nbits, "distance %u", d);
    }

    // one used symbol (with the end of block: two)
    lit.assign(286, 0); lit[65] = 1000;
    check_lengths("one", lit, 15);
    lit[256] = 1;
    write_case(dir, "one_literal", lit, none, true);
    // two used symbols
    lit.assign(286, 0); lit[0] = 7; lit[255] = 9;
    check_lengths("two", lit, 15);
    lit[256] = 1;
    write_case(dir, "two_literals", lit, none, false);
    // all 286 equal
    lit.assign(286, 5); dist.assign(30, 5);
    check_lengths("equal286", lit, 15);
    check_lengths("equal30", dist, 15);
    write_case(dir, "all_equal", lit, dist, true);
    // no distance code, one distance code
    lit.assign(286, 0);
    for (unsigned s = 0; s < 256; s++) lit[s] = 1 + s % 7;
    lit[256] = 1;
    check_lengths("no_distance", none, 15);
    write_case(dir, "no_distance", lit, none, true);
    for (unsigned s = 257; s < 286; s++) lit[s] = 3;
    for (unsigned d : {0u, 13u, 29u}) {
        dist.assign(30, 0); dist[d] = 87;
        check_lengths("one_distance", dist, 15);
        write_case(dir, ("one_distance_" + std::to_string(d)).c_str(), lit, dist, d != 13);
    }
    // Fibonacci counts: deeper than 15 without the limit (24 symbols), deeper than 7 for the 19-symbol code
    lit.assign(286, 0);
    {
        uint32_t a = 1, b = 1;
        for (unsigned s = 0; s < 24; s++) { lit[s * 11] = a; const uint32_t c = a + b; a = b; b = c; }
        uint64_t best; unsigned depth;
        huffman(lit, best, depth);
        CHECK(depth > 15, "the Fibonacci histogram is only %u deep", depth);
        check_lengths("fibonacci24", lit, 15);
        lit[256] = 1;
        dist.assign(30, 0);
        a = 1; b = 1;
        for (unsigned s = 0; s < 30; s++) { dist[s] = a; const uint32_t c = a + b; a = b; b = c; }
        check_lengths("fibonacci30", dist, 15);
        write_case(dir, "fibonacci", lit, none, false);
        std::vector<uint32_t> cl(19, 0);
        a = 1; b = 1;
        for (unsigned s = 0; s < 19; s++) { cl[s] = a; const uint32_t c = a + b; a = b; b = c; }
        huffman(cl, best, depth);
        CHECK(depth > 7, "the 19-symbol Fibonacci histogram is only %u deep", depth);
        check_lengths("fibonacci19", cl, 7);
        for (unsigned used = 9; used <= 19; used++) {
            std::vector<uint32_t> part(cl.begin(), cl.begin() + used);
            part.resize(19, 0);
            check_lengths("fibonacci19_part", part, 7);
        }
    }
    // 256 equal literals: every length but the end of block's is 8, the header is runs of one symbol, and the fixed code competes
    lit.assign(286, 0);
    for (unsigned s = 0; s < 256; s++) lit[s] = 4;
    lit[256] = 1;
    write_case(dir, "flat_lengths", lit, none, true);
    // random histograms
    for (unsigned round = 0; round < 300; round++) {
        const unsigned n = round % 3 == 0 ? 286 : round % 3 == 1 ? 30 : 19, limit = n == 19 ? 7 : 15;
        std::vector<uint32_t> h(n, 0);
        const unsigned shape = (round / 3) % 4;
        for (unsigned s = 0; s < n; s++) {
            const uint32_t r = rnd();
            h[s] = shape == 0 ? r % 1000 : shape == 1 ? (r % 4 == 0 ? r % 50 : 0) : shape == 2 ? 1u << (r % 22) : (r % 3 ? 1 : r % 100000);
        }
        check_lengths("random", h, limit);
        if (n == 286 && round % 15 == 0) {
            for (unsigned s = 0; s < n; s++) h[s] = std::min(h[s], 40u);
            h[256] = 1;
            dist.assign(30, 0);
            for (unsigned s = 0; s < 30; s++) dist[s] = rnd() % 3 == 0 ? 1 + rnd() % 9 : 0;
            dist[rnd() % 30] = 1;
            write_case(dir, ("random_" + std::to_string(round)).c_str(), h, dist, true);
        }
    }
    // the run-length coding's cases: runs of zeros of every length around 3, 10, 11, 138, 139, runs of a length around 3, 6, 7
    for (unsigned run : {1u, 2u, 3u, 4u, 6u, 7u, 8u, 10u, 11u, 12u, 137u, 138u, 139u, 140u, 149u, 200u}) {
        for (unsigned value : {0u, 5u}) {
            std::vector<uint8_t> ll(286, 1), dl(30, 2);
            for (unsigned i = 20; i < 20 + run && i < 286; i++) ll[i] = (uint8_t)value;
            uint16_t rle[316];
            uint32_t freq[19];
            const unsigned count = dc::rle_lengths(ll.data(), 286, dl.data(), 30, rle, freq);
            std::vector<unsigned> back;
            for (unsigned i = 0; i < count; i++) {
                const unsigned s = rle[i] & 31u, x = rle[i] >> 5;
                CHECK(s < 19 && x < (1u << dc::cl_extra_bits(s)) + (dc::cl_extra_bits(s) ? 0u : 1u), "rle symbol");
                if (s < 16) back.push_back(s);
                else if (s == 16) { CHECK(!back.empty(), "16 first"); for (unsigned k = 0; k < x + 3; k++) back.push_back(back.back()); }
                else for (unsigned k = 0; k < x + (s == 17 ? 3u : 11u); k++) back.push_back(0);
            }
            CHECK(back.size() == 316, "rle of run %u of %u: %zu lengths", run, value, back.size());
            for (unsigned i = 0; i < 316; i++) CHECK(back[i] == (i < 286 ? ll[i] : dl[i - 286]), "rle of run %u of %u at %u", run, value, i);
            g_checked++;
        }
    }
    std::printf("%d histograms and run-length cases checked\n", g_checked);
    return 0;
}
