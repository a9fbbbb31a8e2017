// subgraph_fused_cases_check.cpp -- what the library's own planning functions (fora_amd/csrc/fora_attn_plan.h,
// fora_amd/csrc/fora_prop_plan.h) decide for the rows of tests/subgraph_fused_cases.py, without a GPU.  Built with plain g++ by
// tests/test_subgraph_fused_cases_cpu.py and run directly; it answers every line of its standard input with one line:
//   vec <off> <ld> <w> <heads> <elt_bytes>   "<V at the view's own address> <V at an aligned base>": attn_vec_width with the widths
//                                            of the element size, for a 256-byte-aligned buffer plus off elements, and for the
//                                            buffer itself (where the upload of a host operand puts its first element)
//   lg <d>                                   prop_group_lg(d)
//   widths <elt_bytes>                       the three widths of prop_widths_bytes
#include "fora_attn_plan.h"
#include "fora_prop_plan.h"

#include <cstdio>
#include <cstring>

using namespace fora;

int main() {
    alignas(256) static unsigned char buffer[256];
    const uint64_t base = (uint64_t)(uintptr_t)buffer;
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "vec")) {
            unsigned long long off, elt;
            long long ld;
            int w, heads;
            if (scanf("%llu %lld %d %d %llu", &off, &ld, &w, &heads, &elt) != 5 || (elt != 1 && elt != 2 && elt != 4) || w < 1 || heads < 1) return 1;
            const uint32_t *widths = prop_widths_bytes((uint32_t)elt);
            printf("%u %u\n", attn_vec_width(base + off * elt, ld, w, heads, (uint32_t)elt, widths, PROP_NWIDTHS),
                   attn_vec_width(base, ld, w, heads, (uint32_t)elt, widths, PROP_NWIDTHS));
        } else if (!strcmp(what, "lg")) {
            unsigned d;
            if (scanf("%u", &d) != 1) return 1;
            printf("%u\n", prop_group_lg(d));
        } else if (!strcmp(what, "widths")) {
            unsigned elt;
            if (scanf("%u", &elt) != 1 || (elt != 1 && elt != 2 && elt != 4)) return 1;
            const uint32_t *widths = prop_widths_bytes(elt);
            static_assert(PROP_NWIDTHS == 3, "three widths an element size");
            printf("%u %u %u\n", widths[0], widths[1], widths[2]);
        } else {
            return 2;
        }
    }
    return 0;
}
