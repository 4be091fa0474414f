// Surface meshes of a uint8 label volume (gfx950): the naive surface net of the set M of voxels with one value - one vertex per
// active cell of the dual grid, one quad per crossing edge - as stream compaction: a count sweep, a prefix scan, an emit sweep
// (include/volseg_hip.h has the definitions; utilities/meshes.py is the Python layer and the host route that gives the same
// bits).  The order of vertices and quads is part of the contract, so nothing is appended with atomics: every wave writes at
// offsets it reads from the scan.
//
// Cells and chunks.  Cell (k, j, i), 0 <= k <= Z, 0 <= j <= Y, 0 <= i <= X, has the voxels (k-1 | k, j-1 | j, i-1 | i) as corners.
// A row of cells (k, j) is cut into chunks of 64 cells along x; chunk g = (k (Y+1) + j) C + ch, C = ceil((X+1) / 64), so that
// ascending g, then ascending bit, is ascending cell index.  A wave takes the chunks ch of kRowsPerWave consecutive rows of cells
// (k, j0 .. j0 + 7) - a column:
//  * they share voxel rows: 2 x (kRowsPerWave + 1) byte loads per lane, issued together (clamped addresses, no branch between
//    them), instead of 4 per chunk.  One ballot per voxel row gives H = "voxel x = 64 ch + lane is in M" (a voxel outside the
//    volume is not); the corner one voxel back is L = H << 1 with the voxel before the chunk shifted in.  From the eight 64-bit
//    masks of a chunk, which are wave-uniform: active = OR & ~AND, and the quads a cell OWNS (it is the largest-index cell
//    around the edges from its corner (k-1, j-1, i-1) to the next voxel along z, y, x) are L00 ^ L10, L00 ^ L01, L00 ^ H00.  No
//    per-voxel branch.
//  * vs_mesh_count stores per chunk the active mask and the packed count vertices | quads << 31 (vertices stay below 2^31 and
//    quads below 3 x 2^31, so sums of packed words do not carry from one field into the other), and adds the four totals with
//    one int64 atomic per workgroup and figure, spread over kTotalSlots partial totals that a 4-thread launch then sums -
//    integer adds, the same bits in any order; 75 000 workgroups on ONE address cost a third of the sweep.  An exclusive scan
//    in ordinary follow-on launches (reduce kScanTile words to one, twice; scan the top; scan each level below with its tile's
//    offset) turns the counts into offsets in place.  No workgroup ever waits on another.
//  * vs_mesh_emit: lane s < 2 x (kRowsPerWave + 1) first loads the stored mask and offsets of chunk ch of one of the rows of
//    cells (k-1 | k, j0-1 .. j0+7) - they are handed round with v_readlane - and the wave leaves before it reads a label where
//    its own chunks are all empty.  Otherwise it recomputes the masks and skips the empty chunks among its own; the
//    vertex id of cell i of a row of cells is that chunk's offset + popcount(stored mask below bit i), and of cell i - 1 it is
//    that id - 1 (wherever a quad asks for it, the cell is active and hence the one counted just before).  A lane writes its
//    vertex at offset + popcount(active below it) and its quads, z then y then x, at the quad offset + popcount of the three
//    quad masks below it: the stores of a wave are contiguous.
#include "common.h"
#include "prof.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRowsPerWave = 8;                // rows of cells (k, j0 .. j0 + 7) whose chunk ch a wave takes in both sweeps
constexpr int kSlots = kRowsPerWave + 1;       // the voxel rows y = j0 - 1 .. j0 + 7 those share, per z
constexpr int kScanItems = 4;                  // words a thread of the scan holds
constexpr int kScanTile = kThreads * kScanItems;       // words one workgroup reduces or scans: 1024; three levels reach 2^30 chunks
constexpr uint64_t kVertexField = 0x7FFFFFFFull;       // packed word: vertices in bits 0 .. 30, quads from bit 31
constexpr int kTotalSlots = 256;               // partial totals the count sweep's workgroups spread their atomics over

struct Layout {                                // the workspace: masks, packed counts / offsets, the two upper scan levels, the partial totals
    int64_t chunks_per_row, chunks, n1, n2;
    int64_t row_blocks, columns;               // the sweeps: blocks of kRowsPerWave rows of cells per k, and the columns (one per wave)
    size_t bytes;
};

Layout layout_of(int64_t Z, int64_t Y, int64_t X) {
    Layout l;
    l.chunks_per_row = (X + 1 + 63) / 64;
    l.chunks = (Z + 1) * (Y + 1) * l.chunks_per_row;       // every chunk holds at least 2 cells: below 2^30
    l.row_blocks = (Y + 1 + kRowsPerWave - 1) / kRowsPerWave;
    l.columns = (Z + 1) * l.row_blocks * l.chunks_per_row;
    l.n1 = (l.chunks + kScanTile - 1) / kScanTile;
    l.n2 = (l.n1 + kScanTile - 1) / kScanTile;
    l.bytes = (size_t)(2 * l.chunks + l.n1 + l.n2 + 4 * kTotalSlots) * 8;
    return l;
}

// off_a of the smooth style per 8-bit corner mask (bit 4 dz + 2 dy + dx): float32(float64(S_a) / float64(2 n)) over the crossing
// edges; an edge parallel to a adds 1 to S_a and twice its fixed offset (0 or 2) to the other two.  Masks 0 and 255 are not active.
struct SmoothTable {
    float off[256][3];
};

constexpr SmoothTable make_smooth_table() {
    SmoothTable t{};
    for (int m = 0; m < 256; ++m) {
        int s[3] = {0, 0, 0}, n = 0;
        for (int a = 0; a < 3; ++a)                                    // a = 0, 1, 2: z, y, x; corner bit of offset d along a: 4 >> a
            for (int u = 0; u < 2; ++u)
                for (int v = 0; v < 2; ++v) {
                    const int b = (a + 1) % 3, c = (a + 2) % 3;
                    const int lo = u * (4 >> b) + v * (4 >> c), hi = lo + (4 >> a);
                    if (((m >> lo) ^ (m >> hi)) & 1) {
                        ++n;
                        s[a] += 1;
                        s[b] += 2 * u;
                        s[c] += 2 * v;
                    }
                }
        for (int a = 0; a < 3; ++a) t.off[m][a] = n ? (float)((double)s[a] / (double)(2 * n)) : 0.5f;
    }
    return t;
}

__device__ const SmoothTable kSmooth = make_smooth_table();

// ---- a column: chunk ch of the rows of cells (k, j0 .. j0 + kRowsPerWave - 1) -----------------------------------------------------------
struct Column {                                // slot t of z index dz is the voxel row (k-1+dz, j0-1+t)
    uint64_t H[2][kSlots];                     // bit l: voxel x = 64 ch + l of that row is in M
    uint32_t carry[2];                         // bit t: the voxel before the chunk, x = 64 ch - 1, is in M
    __device__ __forceinline__ uint64_t L(int dz, int t) const { return (H[dz][t] << 1) | ((carry[dz] >> t) & 1u); }
};

struct Place {                                 // which column a wave takes
    int k, j0, ch;
};

__device__ __forceinline__ Place place_of(int64_t column, int chunks_per_row, int row_blocks) {
    const int64_t rest = column / chunks_per_row;
    Place p;
    p.ch = (int)(column - rest * chunks_per_row);
    p.k = (int)(rest / row_blocks);
    p.j0 = (int)(rest - (int64_t)p.k * row_blocks) * kRowsPerWave;
    return p;
}

// All loads first, at clamped addresses so that nothing branches between them; what lies outside the volume is masked afterwards.
__device__ __forceinline__ Column load_column(const uint8_t* __restrict__ labels, int Z, int Y, int X, int value, Place p, int lane) {
    const int i0 = p.ch * 64, x = i0 + lane;
    const int x_in = min(x, X - 1), x_before = max(i0 - 1, 0);        // i0 <= X: voxel i0 - 1 is inside the row where i0 > 0
    int here[2][kSlots], before[2][kSlots];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int t = 0; t < kSlots; ++t) {
            const int z = min(max(p.k - 1 + dz, 0), Z - 1), y = min(max(p.j0 - 1 + t, 0), Y - 1);
            const uint8_t* row = labels + ((int64_t)z * Y + y) * X;
            here[dz][t] = row[x_in];
            before[dz][t] = row[x_before];
        }
    Column c;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        c.carry[dz] = 0;
#pragma unroll
        for (int t = 0; t < kSlots; ++t) {
            const int z = p.k - 1 + dz, y = p.j0 - 1 + t;
            const bool inside = z >= 0 && z < Z && y >= 0 && y < Y;    // uniform over the wave
            c.H[dz][t] = __ballot(inside && x < X && here[dz][t] == value);
            c.carry[dz] |= (uint32_t)(inside && i0 > 0 && before[dz][t] == value) << t;
        }
    }
    return c;
}

struct Corners {                               // bit l: the corner of cell 64 ch + l at voxel (k-1+dz, j-1+dy, i-1 | i) is in M
    uint64_t L[2][2], H[2][2];
};

__device__ __forceinline__ Corners corners_of(const Column& c, int t) {       // of the row of cells j0 + t
    Corners r;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            r.H[dz][dy] = c.H[dz][t + dy];
            r.L[dz][dy] = c.L(dz, t + dy);
        }
    return r;
}

__device__ __forceinline__ uint64_t active_of(const Corners& c) {
    const uint64_t any = c.L[0][0] | c.H[0][0] | c.L[0][1] | c.H[0][1] | c.L[1][0] | c.H[1][0] | c.L[1][1] | c.H[1][1];
    const uint64_t all = c.L[0][0] & c.H[0][0] & c.L[0][1] & c.H[0][1] & c.L[1][0] & c.H[1][0] & c.L[1][1] & c.H[1][1];
    return any & ~all;
}

__global__ __launch_bounds__(kThreads) void mesh_count_kernel(const uint8_t* __restrict__ labels, int Z, int Y, int X, int value, int chunks_per_row,
                                                            int row_blocks, int64_t columns, uint64_t* __restrict__ mask,
                                                            uint64_t* __restrict__ packed, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long part[kWaves][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t column = (int64_t)blockIdx.x * kWaves + wave;
    unsigned long long sum[4] = {0, 0, 0, 0};                          // vertices, quads across z, y, x: uniform over the wave
    if (column < columns) {                                            // uniform
        const Place p = place_of(column, chunks_per_row, row_blocks);
        const Column col = load_column(labels, Z, Y, X, value, p, lane);
        uint64_t my_mask = 0, my_packed = 0;                           // lane t keeps the words of the row of cells j0 + t
#pragma unroll
        for (int t = 0; t < kRowsPerWave; ++t) {
            if (p.j0 + t > Y) break;                                   // uniform
            const Corners c = corners_of(col, t);
            const uint64_t act = active_of(c);
            const int v = __popcll(act), qz = __popcll(c.L[0][0] ^ c.L[1][0]), qy = __popcll(c.L[0][0] ^ c.L[0][1]), qx = __popcll(c.L[0][0] ^ c.H[0][0]);
            if (lane == t) {
                my_mask = act;
                my_packed = (uint64_t)v | ((uint64_t)(qz + qy + qx) << 31);
            }
            sum[0] += v; sum[1] += qz; sum[2] += qy; sum[3] += qx;
        }
        if (lane < kRowsPerWave && p.j0 + lane <= Y) {
            const int64_t g = ((int64_t)p.k * (Y + 1) + p.j0 + lane) * chunks_per_row + p.ch;
            mask[g] = my_mask;
            packed[g] = my_packed;
        }
    }
    if (lane < 4) part[wave][lane] = sum[lane];
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(partial + (blockIdx.x % kTotalSlots) * 4 + threadIdx.x, t);       // one address would serialise every workgroup of the sweep
    }
}

__global__ void mesh_totals_kernel(const unsigned long long* __restrict__ partial, long long* __restrict__ totals) {
    unsigned long long t = 0;                                          // 4 threads, one figure each
    for (int slot = 0; slot < kTotalSlots; ++slot) t += partial[slot * 4 + threadIdx.x];
    totals[threadIdx.x] = (long long)t;
}

// ---- the scan: reduce a tile to one word; scan a tile in place, exclusive, from the offset of the level above -------------------------
__device__ __forceinline__ uint64_t wave_inclusive(uint64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)x, d, 64);
        if (lane >= d) x += up;
    }
    return x;
}

__global__ __launch_bounds__(kThreads) void mesh_reduce_kernel(const uint64_t* __restrict__ in, int64_t n, uint64_t* __restrict__ out) {
    __shared__ uint64_t part[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint64_t x = 0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t)
        if (base + t < n) x += in[base + t];
    x = wave_inclusive(x, lane);
    if (lane == 63) part[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += part[w];
        out[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kThreads) void mesh_scan_kernel(uint64_t* __restrict__ data, int64_t n, const uint64_t* __restrict__ offsets) {
    __shared__ uint64_t part[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint64_t item[kScanItems], mine = 0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) {
        item[t] = base + t < n ? data[base + t] : 0;
        mine += item[t];
    }
    const uint64_t incl = wave_inclusive(mine, lane);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint64_t run = offsets ? offsets[blockIdx.x] : 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) run += part[w];
    run += incl - mine;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) {
        if (base + t < n) data[base + t] = run;
        run += item[t];
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t from_lane(uint64_t v, int source) {       // v of lane `source` (a constant), wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, source);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), source);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void mesh_emit_kernel(const uint8_t* __restrict__ labels, int Z, int Y, int X, int value, int blocky,
                                                           int chunks_per_row, int row_blocks, int64_t columns, const uint64_t* __restrict__ mask,
                                                           const uint64_t* __restrict__ packed, float* __restrict__ vertices, int4* __restrict__ quads) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t column = (int64_t)blockIdx.x * kWaves + wave;
    if (column >= columns) return;                                     // uniform; no barrier follows
    const Place p = place_of(column, chunks_per_row, row_blocks);
    const uint64_t below = ((uint64_t)1 << lane) - 1;

    // lane s = dz kSlots + t holds what vs_mesh_count left for chunk ch of the row of cells (k-1+dz, j0-1+t); 0 for a row that does
    // not exist - no quad asks for one.  The wave's own rows are dz = 1, t = 1 .. kRowsPerWave.
    uint64_t stored_mask = 0, stored_word = 0;
    if (lane < 2 * kSlots) {
        const int dz = lane / kSlots, t = lane - dz * kSlots;
        const int kk = p.k - 1 + dz, jj = p.j0 - 1 + t;
        if (kk >= 0 && jj >= 0 && jj <= Y) {
            const int64_t gg = ((int64_t)kk * (Y + 1) + jj) * chunks_per_row + p.ch;
            stored_mask = mask[gg];
            stored_word = packed[gg];
        }
    }
    if (!__ballot(lane > kSlots && lane < 2 * kSlots && stored_mask != 0)) return;      // uniform: no vertex, hence no quad either - most of a volume

    const Column col = load_column(labels, Z, Y, X, value, p, lane);
#pragma unroll
    for (int t = 0; t < kRowsPerWave; ++t) {
        const uint64_t act = from_lane(stored_mask, kSlots + 1 + t);
        if (!act) continue;                                            // uniform; a row of cells beyond Y reads 0 too
        const int j = p.j0 + t;
        const Corners c = corners_of(col, t);
        const uint64_t word = from_lane(stored_word, kSlots + 1 + t);
        const int64_t voff = (int64_t)(word & kVertexField), qoff = (int64_t)(word >> 31);

        int id[2][2];                                                  // the id of cell 64 ch + lane in the rows of cells (k-1 | k, j-1 | j)
#pragma unroll
        for (int dz = 0; dz < 2; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int s = dz * kSlots + t + dy;
                id[dz][dy] = (int)(from_lane(stored_word, s) & kVertexField) + __popcll(from_lane(stored_mask, s) & below);
            }

        if ((act >> lane) & 1) {
            const int i = p.ch * 64 + lane;
            float oz = 0.5f, oy = 0.5f, ox = 0.5f;
            if (!blocky) {
                int m = 0;
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy)
                        m |= (int)((c.L[dz][dy] >> lane) & 1) << (4 * dz + 2 * dy) | (int)((c.H[dz][dy] >> lane) & 1) << (4 * dz + 2 * dy + 1);
                oz = kSmooth.off[m][0]; oy = kSmooth.off[m][1]; ox = kSmooth.off[m][2];
            }
            float* v = vertices + (voff + __popcll(act & below)) * 3;
            v[0] = (float)(p.k - 1) + oz;
            v[1] = (float)(j - 1) + oy;
            v[2] = (float)(i - 1) + ox;
        }

        const uint64_t qz = c.L[0][0] ^ c.L[1][0], qy = c.L[0][0] ^ c.L[0][1], qx = c.L[0][0] ^ c.H[0][0];
        if (((qz | qy | qx) >> lane) & 1) {
            int4* q = quads + qoff + __popcll(qz & below) + __popcll(qy & below) + __popcll(qx & below);
            const bool lower = (c.L[0][0] >> lane) & 1;                // the lower of the two positions is the one in M
            if ((qz >> lane) & 1) {                                    // cells (k, j-1 | j, i-1 | i)
                const int v1 = id[1][0], v3 = id[1][1] - 1;
                *q++ = make_int4(id[1][0] - 1, lower ? v1 : v3, id[1][1], lower ? v3 : v1);
            }
            if ((qy >> lane) & 1) {                                    // cells (k-1 | k, j, i-1 | i)
                const int v1 = id[1][1] - 1, v3 = id[0][1];
                *q++ = make_int4(id[0][1] - 1, lower ? v1 : v3, id[1][1], lower ? v3 : v1);
            }
            if ((qx >> lane) & 1) {                                    // cells (k-1 | k, j-1 | j, i)
                const int v1 = id[0][1], v3 = id[1][0];
                *q++ = make_int4(id[0][0], lower ? v1 : v3, id[1][1], lower ? v3 : v1);
            }
        }
    }
}

int check_common(const char* who, int64_t Z, int64_t Y, int64_t X, int value, size_t workspace_bytes, Layout* l) {
    VS_REQUIRE(extents_fit(Z, Y, X, 1), "%s: extents %lld x %lld x %lld - every extent must be at least 1 and the (Z+1)(Y+1)(X+1) cells below 2^31 "
               "(vertex ids are int32)", who, (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(value >= 0 && value <= 255, "%s: value %d is not a uint8 value", who, value);
    *l = layout_of(Z, Y, X);
    VS_REQUIRE(workspace_bytes >= l->bytes, "%s: workspace of %zu bytes, vs_mesh_workspace_bytes asks for %zu", who, workspace_bytes, l->bytes);
    return VS_OK;
}

unsigned sweep_groups(const Layout& l) { return (unsigned)((l.columns + kWaves - 1) / kWaves); }       // a column per wave

}  // namespace

extern "C" size_t vs_mesh_workspace_bytes(int64_t Z, int64_t Y, int64_t X) {
    return extents_fit(Z, Y, X, 1) ? layout_of(Z, Y, X).bytes : 0;
}

extern "C" int vs_mesh_count(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int value, void* workspace, size_t workspace_bytes,
                             int64_t* totals, void* stream) {
    Layout l;
    if (int rc = check_common("mesh_count", Z, Y, X, value, workspace_bytes, &l)) return rc;
    VS_REQUIRE(labels && workspace && totals, "mesh_count: null argument");
    VS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)totals % 8 == 0, "mesh_count: workspace and totals must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint64_t* mask = (uint64_t*)workspace;
    uint64_t *packed = mask + l.chunks, *s1 = packed + l.chunks, *s2 = s1 + l.n1, *partial = s2 + l.n2;
    VS_CHECK_HIP(hipMemsetAsync(partial, 0, 4 * kTotalSlots * sizeof(uint64_t), s));
    {
        ProfScope prof(PK_POOL_MISC, 0.0, (double)Z * Y * X + 16.0 * (double)l.chunks, s);      // every voxel once from memory, a mask and a count per chunk
        hipLaunchKernelGGL(mesh_count_kernel, dim3(sweep_groups(l)), dim3(kThreads), 0, s, labels, (int)Z, (int)Y, (int)X, value,
                           (int)l.chunks_per_row, (int)l.row_blocks, l.columns, mask, packed, (unsigned long long*)partial);
        VS_LAUNCH_CHECK();
        hipLaunchKernelGGL(mesh_totals_kernel, dim3(1), dim3(4), 0, s, (const unsigned long long*)partial, (long long*)totals);
        VS_LAUNCH_CHECK();
    }
    // counts -> exclusive offsets, in place: up two levels where there is more than one tile, then down
    if (l.n1 > 1) {
        hipLaunchKernelGGL(mesh_reduce_kernel, dim3((unsigned)l.n1), dim3(kThreads), 0, s, packed, l.chunks, s1);
        VS_LAUNCH_CHECK();
        if (l.n2 > 1) {
            hipLaunchKernelGGL(mesh_reduce_kernel, dim3((unsigned)l.n2), dim3(kThreads), 0, s, s1, l.n1, s2);
            VS_LAUNCH_CHECK();
            hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kThreads), 0, s, s2, l.n2, (const uint64_t*)nullptr);     // n2 <= kScanTile: chunks < 2^30
            VS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(mesh_scan_kernel, dim3((unsigned)l.n2), dim3(kThreads), 0, s, s1, l.n1, l.n2 > 1 ? (const uint64_t*)s2 : nullptr);
        VS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mesh_scan_kernel, dim3((unsigned)l.n1), dim3(kThreads), 0, s, packed, l.chunks, l.n1 > 1 ? (const uint64_t*)s1 : nullptr);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_mesh_emit(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int value, int style, const void* workspace,
                            size_t workspace_bytes, float* vertices, int32_t* quads, void* stream) {
    Layout l;
    if (int rc = check_common("mesh_emit", Z, Y, X, value, workspace_bytes, &l)) return rc;
    VS_REQUIRE(style == VS_MESH_SMOOTH || style == VS_MESH_BLOCKY, "mesh_emit: style %d - it is VS_MESH_SMOOTH (0) or VS_MESH_BLOCKY (1)", style);
    if (!vertices && !quads) return VS_OK;                             // the caller read totals of 0: nothing to emit, no launch
    VS_REQUIRE(labels && workspace && vertices && quads, "mesh_emit: null argument");
    VS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)vertices % 4 == 0 && (uintptr_t)quads % 16 == 0,
               "mesh_emit: the workspace must be 8-byte, vertices 4-byte and quads 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* mask = (const uint64_t*)workspace;
    ProfScope prof(PK_POOL_MISC, 0.0, (double)Z * Y * X + 16.0 * (double)l.chunks, s);          // plus the outputs, which only the caller can size
    hipLaunchKernelGGL(mesh_emit_kernel, dim3(sweep_groups(l)), dim3(kThreads), 0, s, labels, (int)Z, (int)Y, (int)X, value,
                       style == VS_MESH_BLOCKY ? 1 : 0, (int)l.chunks_per_row, (int)l.row_blocks, l.columns, mask, mask + l.chunks, vertices,
                       (int4*)quads);
    VS_LAUNCH_CHECK();
    return VS_OK;
}
