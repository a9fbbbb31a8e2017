// walk_dg_lds_tables.cpp -- the bytes of k_walk_dg's tables in dynamic LDS for one graph, from fora_amd/csrc/fora_tables.h on the
// CPU: make_walk_dg builds the degree-grouped copy, walk_dg_lds_bytes is the size the launch passes.  Stand-alone
// (tests/test_walk_dg_lds_cpu.py compiles it):
//
//   walk_dg_lds_tables <csr file>
//
// The file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col[nnz], little-endian.  One line "key=value ...".
#include "fora_tables.h"

#include <cstdio>

using namespace fora;

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: %s <csr file>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    int64_t head[2];
    if (!f || std::fread(head, 8, 2, f) != 2 || head[0] <= 0 || head[0] >= (1 << 24) || head[1] < 0 || head[1] >= (1ll << 28)) { std::printf("bad graph file\n"); return 1; }
    std::vector<int64_t> row_ptr((size_t)head[0] + 1);
    std::vector<int32_t> col((size_t)head[1]);
    if (std::fread(row_ptr.data(), 8, row_ptr.size(), f) != row_ptr.size() || std::fread(col.data(), 4, col.size(), f) != col.size()) { std::printf("short graph file\n"); return 1; }
    std::fclose(f);
    const DgTables t = make_walk_dg((int32_t)head[0], row_ptr.data(), col.data(), 0);
    const uint32_t nblk = (uint32_t)t.T.size();
    std::printf("have=%d H=%u nrec=%u nblk=%u nbx=%u lds_xl=%zu lds_plain=%zu\n", (int)t.have, t.H, t.nrec, nblk, t.nbx,
                walk_dg_lds_bytes(t.H, t.nrec, nblk, true), walk_dg_lds_bytes(t.H, t.nrec, nblk, false));
    return 0;
}
