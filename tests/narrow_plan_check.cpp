// narrow_plan_check.cpp -- the host side of NARROW OPERANDS (fora_amd/csrc/fora_narrow.h, the one-byte width table of
// fora_amd/csrc/fora_prop_plan.h) against restatements, without a GPU.  Built with -fsanitize=address,undefined by
// tests/test_narrow_cpu.py and run directly.
//
//   narrow_plan_check decode   the three decoders on every code against ldexp; elt_bytes and elt_known; prints
//                              "codes=<count> ok"
//   narrow_plan_check geom     prop_geom and attn_vec_width with 1-byte elements and the one-byte table over addresses 0 .. 31,
//                              pitches 1 .. 40 and d 1 .. 40 against brute force; prints "cases=<count> ok"
//   narrow_plan_check bytes    prop_matrix_bytes with element size 1; prints "ok"
#include "fora_attn_plan.h"
#include "fora_narrow.h"
#include "fora_prop_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace fora;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static float as_float(uint32_t bits) { float f; memcpy(&f, &bits, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// the rule of include/fora_hip.h in ldexp; nan: the code is a NaN
static float f16_rule(uint32_t h, bool &nan) {
    const int s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
    nan = e == 31 && m != 0;
    float v;
    if (e == 31) v = m ? NAN : INFINITY;
    else if (e == 0) v = ldexpf((float)m, -24);
    else v = ldexpf((float)(1024 + m), e - 25);
    return s ? -v : v;
}
static float e4m3_rule(uint32_t b, bool &nan) {
    const int s = (b >> 7) & 1, e = (b >> 3) & 15, m = b & 7;
    nan = (b & 0x7F) == 0x7F;
    float v;
    if (nan) v = NAN;
    else if (e == 0) v = ldexpf((float)m, -9);
    else v = ldexpf((float)(8 + m), e - 10);
    return s ? -v : v;
}
// equal bits (so -0 is -0), or both NaN with the decoder's a quiet one
static bool same(uint32_t got, float want, bool nan) {
    if (nan) return (got & 0x7FC00000u) == 0x7FC00000u;
    return got == as_bits(want);
}

static int decode() {
    static_assert(narrow_f16_bits(0x3C00u) == 0x3F800000u && narrow_e4m3_bits(0x38u) == 0x3F800000u && narrow_e5m2_bits(0x3Cu) == 0x3F800000u, "1.0");
    static_assert(narrow_e4m3_bits(0x7Eu) == 0x43E00000u, "448");
    uint64_t count = 0;
    bool nan = false;
    for (uint32_t h = 0; h < 65536; h++, count++) {
        const float want = f16_rule(h, nan);
        CHECK(same(narrow_f16_bits(h), want, nan));
        CHECK(narrow_bits(ELT_F16, h) == narrow_f16_bits(h));
    }
    for (uint32_t b = 0; b < 256; b++, count += 2) {
        float want = f16_rule(b << 8, nan);
        CHECK(same(narrow_e5m2_bits(b), want, nan));
        CHECK(narrow_bits(ELT_E5M2, b) == narrow_e5m2_bits(b));
        want = e4m3_rule(b, nan);
        CHECK(same(narrow_e4m3_bits(b), want, nan));
        CHECK(narrow_bits(ELT_E4M3, b) == narrow_e4m3_bits(b));
    }
    CHECK(as_float(narrow_e4m3_bits(0x7E)) == 448.0f && as_float(narrow_e4m3_bits(0xFE)) == -448.0f);
    CHECK(narrow_f16_bits(0x8000u) == 0x80000000u && narrow_e4m3_bits(0x80u) == 0x80000000u && narrow_e5m2_bits(0x80u) == 0x80000000u);
    CHECK(elt_bytes(ELT_F32) == 4 && elt_bytes(ELT_BF16) == 2 && elt_bytes(ELT_F16) == 2 && elt_bytes(ELT_E4M3) == 1 && elt_bytes(ELT_E5M2) == 1);
    for (int t = -2; t < 10; t++) CHECK(elt_known(t) == (t == 0 || t == 1 || t == 4 || t == 5 || t == 6));
    printf("codes=%llu ok\n", (unsigned long long)count);
    return 0;
}

static bool qualifies(uint32_t V, uint64_t addr, int64_t ld, int d) { return V == 1 || (V <= (uint32_t)d && addr % V == 0 && ld % (int64_t)V == 0); }

static int geom() {
    const uint32_t *w = prop_widths_bytes(1);
    CHECK(prop_widths_bytes(4) == prop_widths(false) && prop_widths_bytes(2) == prop_widths(true));
    for (int i = 0; i + 1 < PROP_NWIDTHS; i++) CHECK(w[i] > w[i + 1]);
    CHECK(w[PROP_NWIDTHS - 1] == 1 && w[0] <= 16);
    uint64_t count = 0;
    for (uint64_t addr = 0; addr < 32; addr++)
        for (int64_t ld = 1; ld <= 40; ld++)
            for (int d = 1; d <= 40; d++, count++) {
                const PropGeom g = prop_geom(addr, ld, d, 1, w, PROP_NWIDTHS);
                CHECK(ld % g.V == 0 && addr % g.V == 0 && g.V <= (uint32_t)d && g.V <= 16);
                bool in_table = false;
                for (int i = 0; i < PROP_NWIDTHS; i++) {
                    in_table |= w[i] == g.V;
                    if (w[i] > g.V) CHECK(!qualifies(w[i], addr, ld, d)); // no wider width of the table qualifies
                }
                CHECK(in_table);
                // the lanes: G a power of two that holds the row's lanes, tiles of G * V columns that cover d
                const uint32_t lanes = ((uint32_t)d + g.V - 1) / g.V;
                CHECK(g.G >= 1 && g.G <= 64 && (g.G & (g.G - 1)) == 0 && g.segs_per_wave == 64 / g.G);
                CHECK((uint64_t)g.tiles * g.G >= lanes && (uint64_t)(g.tiles - 1) * g.G < lanes);
                CHECK(g.G == 64 || g.G >= lanes);
                // a head's slice: every head's first column must keep the alignment, so V divides dv as well
                for (int heads = 1; heads <= 3; heads++) {
                    const uint32_t V = attn_vec_width(addr, ld, d, heads, 1, w, PROP_NWIDTHS);
                    CHECK(qualifies(V, addr, ld, d) && V <= 16);
                    if (heads > 1) CHECK(d % (int)V == 0);
                    for (int i = 0; i < PROP_NWIDTHS; i++)
                        if (w[i] > V) CHECK(!(qualifies(w[i], addr, ld, d) && (heads == 1 || d % (int)w[i] == 0)));
                }
            }
    printf("cases=%llu ok\n", (unsigned long long)count);
    return 0;
}

static int bytes() {
    CHECK(prop_matrix_bytes(0, 40, 33, 1) == 0);
    CHECK(prop_matrix_bytes(1, 40, 33, 1) == 33);
    CHECK(prop_matrix_bytes(2000, 40, 33, 1) == 1999ull * 40 + 33);
    CHECK(prop_matrix_bytes(2000, 16, 16, 1) == 32000);
    CHECK(prop_matrix_bytes(3, 7, 5, 1) * 2 == prop_matrix_bytes(3, 7, 5, 2) && prop_matrix_bytes(3, 7, 5, 1) * 4 == prop_matrix_bytes(3, 7, 5, 4));
    CHECK(prop_vector_bytes(9, 1) == 9);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "decode")) return decode();
    if (argc == 2 && !strcmp(argv[1], "geom")) return geom();
    if (argc == 2 && !strcmp(argv[1], "bytes")) return bytes();
    printf("usage: narrow_plan_check decode | geom | bytes\n");
    return 2;
}
