// softmax_exp_check.cpp -- exp_def (fora_amd/csrc/fora_softmax_exp.h, the exponential of ROW SOFTMAX) on the CPU: the header as
// the library compiles it, in a stand-alone program.  Reads a file of points, one per line as the 16 hex digits of the double's
// bits, and prints the bits of exp_def of each in the same form.  tests/test_softmax_cpu.py builds it with
// -ffp-contract=off under the address and undefined-behaviour sanitizers and holds the output to the numpy twin.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fora_softmax_exp.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: softmax_exp_check <file of hex words>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> words;
    uint64_t w;
    while (fscanf(f, "%" SCNx64, &w) == 1) words.push_back(w);
    fclose(f);
    for (uint64_t bits : words) {
        double t, e;
        memcpy(&t, &bits, 8);
        e = fora::exp_def(t);
        memcpy(&bits, &e, 8);
        printf("%016" PRIx64 "\n", bits);
    }
    return 0;
}
