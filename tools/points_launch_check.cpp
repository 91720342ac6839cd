// Stand-alone check of the point-feature launchers' host arithmetic (vtaco_amd/csrc/points_launch.h): walks the index maps of
// point_sample.hip's kernels on the host, over the shapes the GPU tests use and the 128^3 lattice, writing through real buffers of
// the sizes the launchers allocate -- so a tile count, a last partial tile or a workspace size that is off shows as a wrong
// coverage count here or as an out-of-bounds access under the sanitizers.
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vtaco_amd/csrc tools/points_launch_check.cpp -o /tmp/points_launch_check && /tmp/points_launch_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "points_launch.h"

using namespace vt_points;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the forward's grid over (B, M, C): every (b, m, channel) is written once; every cloud row is read once per query
static void check_fwd(int B, int64_t M, int64_t N, int C) {
    const Channels ch = channels_of(C);
    EXPECT(ch.ncb >= 1 && ch.ncb <= MAX_NCB && ch.ncb * ch.groups * 32 == C, "channels_of(%d) = %d x %d", C, ch.ncb, ch.groups);
    const int64_t tiles = row_tiles(M);
    EXPECT(grid_ok(tiles, ch.groups, B), "grid (%lld, %d, %d)", (long long)tiles, ch.groups, B);
    std::vector<unsigned char> out((size_t)B * M * C, 0);
    for (int b = 0; b < B; ++b)
        for (int cg = 0; cg < ch.groups; ++cg)
            for (int64_t bx = 0; bx < tiles; ++bx)
                for (int wave = 0; wave < WAVES; ++wave)
                    for (int l32 = 0; l32 < ROWS_PER_WAVE; ++l32) {
                        const int64_t m = bx * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE + l32;
                        if (m >= M) continue;
                        for (int cb = 0; cb < ch.ncb; ++cb)
                            for (int c = 0; c < 32; ++c) ++out[((size_t)b * M + m) * C + (size_t)cg * ch.ncb * 32 + cb * 32 + c];
                    }
    for (unsigned char v : out) if (v != 1) { EXPECT(false, "forward B=%d M=%lld C=%d: an output written %d times", B, (long long)M, C, v); break; }
    std::vector<unsigned char> seen((size_t)N, 0);
    for (int64_t t = 0; t < k_tiles(N); ++t)
        for (int j = 0; j < TILE_K; ++j)
            if (t * TILE_K + j < N) ++seen[(size_t)(t * TILE_K + j)];
    for (unsigned char v : seen) if (v != 1) { EXPECT(false, "forward N=%lld: a cloud point visited %d times", (long long)N, v); break; }
}

// the backward's chunks: every query lands in one chunk, the partial sums fit the workspace, every gradient element is written
static void check_bwd(int B, int64_t M, int64_t N, int C) {
    const Channels ch = channels_of(C);
    const int64_t chunks = bwd_chunks(M), tiles = row_tiles(N);
    EXPECT(grid_ok(tiles, chunks * ch.groups, B), "bwd grid (%lld, %lld, %d)", (long long)tiles, (long long)(chunks * ch.groups), B);
    const size_t bytes = bwd_workspace_bytes(B, M, N, C);
    EXPECT((chunks > 1) == (bytes > 0), "workspace %zu bytes for %lld chunks", bytes, (long long)chunks);
    std::vector<unsigned char> q((size_t)M, 0);
    for (int64_t k = 0; k < chunks; ++k) {
        EXPECT(bwd_chunk_lo(k) % TILE_K == 0, "chunk %lld starts off a tile", (long long)k);
        for (int64_t m0 = bwd_chunk_lo(k); m0 < bwd_chunk_hi(k, M); m0 += TILE_K)
            for (int j = 0; j < TILE_K; ++j)
                if (m0 + j < bwd_chunk_hi(k, M)) ++q[(size_t)(m0 + j)];
    }
    for (unsigned char v : q) if (v != 1) { EXPECT(false, "backward M=%lld: a query in %d chunks", (long long)M, v); break; }
    std::vector<unsigned char> dst(chunks > 1 ? bytes / sizeof(float) : (size_t)B * N * C, 0);
    for (int64_t k = 0; k < chunks; ++k)
        for (int b = 0; b < B; ++b)
            for (int cg = 0; cg < ch.groups; ++cg)
                for (int64_t bx = 0; bx < tiles; ++bx)
                    for (int r = 0; r < ROWS_PER_BLOCK; ++r) {
                        const int64_t n = bx * ROWS_PER_BLOCK + r;
                        if (n >= N) continue;
                        for (int c = 0; c < ch.ncb * 32; ++c) ++dst[(((size_t)k * B + b) * N + n) * C + (size_t)cg * ch.ncb * 32 + c];
                    }
    for (unsigned char v : dst) if (v != 1) { EXPECT(false, "backward B=%d M=%lld N=%lld C=%d: a partial sum written %d times", B, (long long)M, (long long)N, C, v); break; }
}

int main() {
    const int64_t Ms[] = {1, 31, 32, 33, 67, 127, 128, 129, 257, 511, 512, 513, 1024, 1100, 2048};
    const int64_t Ns[] = {1, 3, 31, 32, 33, 65, 513, 600, 3000};
    for (int C = 32; C <= MAX_C; C += 32)
        for (int64_t M : Ms)
            for (int64_t N : Ns) {
                if (C > 128 && (M > 513 || N > 513)) continue;         // the wide widths at the small shapes: same maps, less time
                check_fwd(2, M, N, C);
                check_bwd(2, M, N, C);
            }
    check_fwd(1, (int64_t)1 << 20, 3000, 32);                          // one slab of the 128^3 lattice (LATTICE_SLAB_POINTS)
    EXPECT(grid_ok(row_tiles((int64_t)128 * 128 * 128), 1, 1), "the whole 128^3 lattice in one launch");
    EXPECT(bwd_workspace_bytes(1, 2048, 3000, 32) == (size_t)4 * 3000 * 32 * 4, "2048 training queries: 4 chunks");
    EXPECT(!c_ok(0) && !c_ok(48) && !c_ok(288) && c_ok(32) && c_ok(256), "c_ok");
    for (int nx : {8, 17}) {
        const int64_t all = (int64_t)nx * nx * nx, nn = (int64_t)nx * nx;
        EXPECT(lattice_ok(nx, 0, all) && lattice_ok(nx, 5, nx == 8 ? all - 5 : 1000) && lattice_ok(nx, nn + 3, 2 * nn + 7), "slabs of %d^3", nx);
        EXPECT(!lattice_ok(nx, 1, all) && !lattice_ok(nx, -1, 4) && !lattice_ok(nx, all, 1) && lattice_ok(nx, all, 0), "slabs outside %d^3", nx);
    }
    EXPECT(!lattice_ok(1, 0, 1) && !lattice_ok(MAX_NX + 1, 0, 1) && lattice_ok(MAX_NX, 0, (int64_t)MAX_NX * MAX_NX * MAX_NX), "nx limits");
    std::printf(failures ? "%d failure(s)\n" : "points_launch_check: ok\n", failures);
    return failures ? 1 : 0;
}
