// Host arithmetic of the point-feature launchers (point_sample.hip, pointnetpp.hip): tile counts, channel grouping, the backward's
// query chunks and the lattice-range check.  Plain C++ with no HIP in it, so a stand-alone program can walk it over shapes
// (tools/points_launch_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vt_points {

constexpr int ROWS_PER_WAVE = 32;        // one 32x32x2 MFMA column block: 32 queries (forward) or 32 cloud points (backward)
constexpr int WAVES = 4;
constexpr int ROWS_PER_BLOCK = ROWS_PER_WAVE * WAVES;
constexpr int TILE_K = 32;               // reduction rows staged in LDS per step: cloud points (forward), queries (backward)
constexpr int MAX_NCB = 4;               // 32-channel blocks one workgroup accumulates (64 accumulator registers)
constexpr int BWD_CHUNK = 512;           // queries per partial sum of the backward; a multiple of TILE_K
constexpr int MAX_C = 256;
constexpr int MAX_NX = 1625;             // 1625^3 < 2^32 <= 1626^3
static_assert(BWD_CHUNK % TILE_K == 0, "a chunk is whole tiles");

// C = 32 * blocks; a workgroup takes ncb of them and gridDim.y = groups covers the rest: ncb * groups == blocks exactly
struct Channels {
    int ncb, groups;
};
inline Channels channels_of(int C) {
    const int blocks = C / 32;
    for (int ncb = MAX_NCB; ncb > 1; --ncb)
        if (blocks % ncb == 0) return {ncb, blocks / ncb};
    return {1, blocks};
}

inline bool c_ok(int C) { return C > 0 && (C & 31) == 0 && C <= MAX_C; }

inline int64_t row_tiles(int64_t rows) { return (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }
inline int64_t k_tiles(int64_t k) { return (k + TILE_K - 1) / TILE_K; }

// the slab [first, first + count) of the nx^3 lattice
inline bool lattice_ok(int nx, int64_t first, int64_t count) {
    if (nx < 2 || nx > MAX_NX || first < 0 || count < 0) return false;
    const int64_t all = (int64_t)nx * nx * nx;
    return first <= all && count <= all - first;
}

// backward: the M queries in chunks of BWD_CHUNK; more than one chunk goes through [chunks][B][N][C] partial sums
inline int64_t bwd_chunks(int64_t M) { return M <= 0 ? 1 : (M + BWD_CHUNK - 1) / BWD_CHUNK; }
inline int64_t bwd_chunk_lo(int64_t chunk) { return chunk * BWD_CHUNK; }
inline int64_t bwd_chunk_hi(int64_t chunk, int64_t M) { const int64_t hi = (chunk + 1) * BWD_CHUNK; return hi < M ? hi : M; }
inline size_t bwd_workspace_bytes(int B, int64_t M, int64_t N, int C) {
    if (B <= 0 || M < 0 || N < 0 || !c_ok(C)) return 0;
    const int64_t chunks = bwd_chunks(M);
    return chunks > 1 ? (size_t)chunks * (size_t)B * (size_t)N * (size_t)C * sizeof(float) : 0;
}

// the launch grids stay inside HIP's limits: x < 2^31, y and z <= 65535
inline bool grid_ok(int64_t x, int64_t y, int64_t z) { return x >= 1 && x < ((int64_t)1 << 31) && y >= 1 && y <= 65535 && z >= 1 && z <= 65535; }

}  // namespace vt_points
