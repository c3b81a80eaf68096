// The mask cleaner: connected components of a uint8 label map, per class the components that are kept, and for every
// pixel that is not kept the class of the nearest kept pixel.  Integers from end to end; every result is a minimum, an integer sum or a
// comparison with a stated tie rule, so no output bit depends on the order in which an atomic arrives.
//
// No workgroup ever waits for another: the phases are kernels.  parent[] holds, per image, linear indices y W + x (-1: no component).
//   label     one workgroup per MC_TILE x MC_TILE tile: union-find in LDS over the tile's pixels, then parent[p] = the tile-local root
//             (the smallest index of the piece), tinfo[root] = the piece's area and whether it touches the frame, ginfo[p] = 0
//   merge     one lane per pixel; a pixel on a tile's rim joins its piece to the equal-label neighbours in other tiles with the
//             min-union of union_find.h on the global array.  Workgroups on different XCDs update the same words here, so every access
//             to parent[] in this kernel is an agent-scope atomic (a plain load could return a stale line of this CU's L1 or this
//             XCD's L2; an atomic load that is late still returns an ancestor)
//   flatten   one lane per pixel: parent[p] = the root (the component's id), and each tile-local root adds its piece to ginfo[root]
//   best      per image and class: components, pixels, pixels of the components that touch the frame, and max (area, -id)
//   keep      out[p] = the label where the pixel's component is kept, 255 elsewhere
//   column    the column pass of seg_dist.h over `out`, per class; its first workgroups also write the stats known so far
//   row       only rows with a pixel that is not kept: min over x' of (x - x')^2 + g^2, per class in ascending order with a strict
//             comparison (a tie stays with the lower class)
#include "seg_dist.h"
#include "union_find.h"

namespace {

constexpr int MC_MAX_CLS = 16;
constexpr int MC_TILE = 32;                                  // tile side: 1024 pixels, four per lane
constexpr int MC_THREADS = 256;
constexpr int MC_TILE_PIX = MC_TILE * MC_TILE;
constexpr int MC_AREA_MASK = 0x00FFFFFF;                     // tinfo / ginfo: the area (at most 2^20) ...
constexpr int MC_FRAME_BIT = 0x40000000;                     // ... and "touches the first or last row or column"
constexpr int MC_BEST_BLOCKS = 32;                           // workgroups per image of the `best` launch at most
constexpr uint8_t MC_NOT_KEPT = 255;
enum { MC_ALL = 0, MC_LARGEST = 1, MC_FRAME = 2 };

struct McModes { uint8_t m[MC_MAX_CLS]; };
// per (image, class), accumulated by `best`: key = area << 32 | ~id of the best component so far
struct McAcc { unsigned long long key; int ncomp, before, frame, pad; };

struct LdsParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct GlobalParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return atomicMin(p + i, v); }
};

// ---------------------------------------------------------------------------------------- components
// grid (ceil(W / 32), ceil(H / 32), N), 256 threads.  INFO: tinfo / ginfo / acc are written too (s2e_mask_clean)
template <bool INFO>
__global__ __launch_bounds__(MC_THREADS) void mc_label_kernel(const uint8_t* __restrict__ labels, int H, int W, int ncls, int conn, int* __restrict__ parent,
                                                              int* __restrict__ tinfo, int* __restrict__ ginfo, McAcc* __restrict__ acc) {
    __shared__ int s_lab[MC_TILE_PIX], s_par[MC_TILE_PIX], s_info[MC_TILE_PIX];
    const int x0 = blockIdx.x * MC_TILE, y0 = blockIdx.y * MC_TILE, n = blockIdx.z;
    const size_t img = (size_t)n * H * W;
    if (INFO && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < MC_MAX_CLS) acc[(size_t)n * MC_MAX_CLS + threadIdx.x] = McAcc{0ull, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < MC_TILE_PIX / MC_THREADS; ++k) {
        const int i = k * MC_THREADS + threadIdx.x, y = y0 + i / MC_TILE, x = x0 + i % MC_TILE;
        const int l = (y < H && x < W) ? (int)labels[img + (size_t)y * W + x] : 255;
        s_lab[i] = l;
        s_par[i] = l < ncls ? i : -1;
        s_info[i] = 0;
    }
    __syncthreads();
    LdsParents lds{s_par};
#pragma unroll
    for (int k = 0; k < MC_TILE_PIX / MC_THREADS; ++k) {
        const int i = k * MC_THREADS + threadIdx.x, ly = i / MC_TILE, lx = i % MC_TILE, l = s_lab[i];
        if (l >= ncls) continue;
        uf_back_neighbours(conn, [&](int dx, int dy) {
            const int qx = lx + dx, qy = ly + dy;
            if (qx >= 0 && qx < MC_TILE && qy >= 0 && s_lab[qy * MC_TILE + qx] == l) uf_union<false>(lds, i, qy * MC_TILE + qx);
        });
    }
    __syncthreads();
    int root[MC_TILE_PIX / MC_THREADS];
#pragma unroll
    for (int k = 0; k < MC_TILE_PIX / MC_THREADS; ++k) {
        const int i = k * MC_THREADS + threadIdx.x, y = y0 + i / MC_TILE, x = x0 + i % MC_TILE;
        root[k] = -1;
        if (s_lab[i] < ncls) {
            root[k] = uf_find(lds, i);
            if (INFO) {
                atomicAdd(&s_info[root[k]], 1);
                if (y == 0 || x == 0 || y == H - 1 || x == W - 1) atomicOr(&s_info[root[k]], MC_FRAME_BIT);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MC_TILE_PIX / MC_THREADS; ++k) {
        const int i = k * MC_THREADS + threadIdx.x, y = y0 + i / MC_TILE, x = x0 + i % MC_TILE;
        if (y < H && x < W) {
            const size_t p = img + (size_t)y * W + x;
            parent[p] = root[k] < 0 ? -1 : (y0 + root[k] / MC_TILE) * W + x0 + root[k] % MC_TILE;
            if (INFO) {
                tinfo[p] = root[k] == i ? s_info[i] : 0;
                ginfo[p] = 0;
            }
        }
    }
}

// grid (ceil(W / 256), H, N), one lane per pixel; only the pixels with a backward neighbour in another tile have work
__global__ __launch_bounds__(MC_THREADS) void mc_merge_kernel(const uint8_t* __restrict__ labels, int H, int W, int ncls, int conn, int* parent) {
    const int x = blockIdx.x * MC_THREADS + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= W) return;
    const bool left = x % MC_TILE == 0, top = y % MC_TILE == 0, right = (x + 1) % MC_TILE == 0;
    if (!left && !top && !(right && conn == 8)) return;
    const size_t img = (size_t)n * H * W;
    const uint8_t* lab = labels + img;
    const int l = lab[(size_t)y * W + x];
    if (l >= ncls) return;
    GlobalParents g{parent + img};
    uf_back_neighbours(conn, [&](int dx, int dy) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0) return;
        if (qx / MC_TILE == x / MC_TILE && qy / MC_TILE == y / MC_TILE) return;      // the tile's own launch has joined these
        if (lab[(size_t)qy * W + qx] == l) uf_union<true>(g, y * W + x, qy * W + qx);
    });
}

// grid (ceil(H W / 256), N), one lane per pixel.  In place: a lane that passes through a word another lane has already flattened reads
// a root, one that reads the word before reads an ancestor; roots do not change in this launch.
template <bool INFO>
__global__ __launch_bounds__(MC_THREADS) void mc_flatten_kernel(int HW, int* parent, const int* __restrict__ tinfo, int* __restrict__ ginfo) {
    const int q = blockIdx.x * MC_THREADS + threadIdx.x, n = blockIdx.y;
    if (q >= HW) return;
    const size_t img = (size_t)n * HW;
    GlobalParents g{parent + img};
    const int v = g.load(q);
    if (v < 0) return;
    const int root = uf_find(g, v);
    if (root != v) g.fetch_min(q, root);
    if (INFO) {
        const int t = tinfo[img + q];
        if (t) {
            atomicAdd(&ginfo[img + root], t & MC_AREA_MASK);
            if (t & MC_FRAME_BIT) atomicOr(&ginfo[img + root], MC_FRAME_BIT);
        }
    }
}

// ---------------------------------------------------------------------------------------- what is kept
// grid (blocks <= MC_BEST_BLOCKS, N): the roots of image n, counted per class in LDS, then one atomic per class and field
__global__ __launch_bounds__(MC_THREADS) void mc_best_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp, const int* __restrict__ ginfo,
                                                             int HW, int ncls, McAcc* __restrict__ acc) {
    __shared__ unsigned long long s_key[MC_MAX_CLS];
    __shared__ int s_n[MC_MAX_CLS], s_before[MC_MAX_CLS], s_frame[MC_MAX_CLS];
    if (threadIdx.x < MC_MAX_CLS) { s_key[threadIdx.x] = 0ull; s_n[threadIdx.x] = 0; s_before[threadIdx.x] = 0; s_frame[threadIdx.x] = 0; }
    __syncthreads();
    const int n = blockIdx.y;
    const size_t img = (size_t)n * HW;
    for (int q = blockIdx.x * MC_THREADS + threadIdx.x; q < HW; q += gridDim.x * MC_THREADS) {
        if (comp[img + q] != q) continue;                    // (-1 for a pixel of no component)
        const int c = labels[img + q], info = ginfo[img + q], area = info & MC_AREA_MASK;
        atomicAdd(&s_n[c], 1);
        atomicAdd(&s_before[c], area);
        if (info & MC_FRAME_BIT) atomicAdd(&s_frame[c], area);
        atomicMax(&s_key[c], (unsigned long long)area << 32 | (0xFFFFFFFFu - (uint32_t)q));      // larger area first, then the smaller id
    }
    __syncthreads();
    if ((int)threadIdx.x < ncls && s_n[threadIdx.x]) {
        McAcc* a = acc + (size_t)n * MC_MAX_CLS + threadIdx.x;
        atomicAdd(&a->ncomp, s_n[threadIdx.x]);
        atomicAdd(&a->before, s_before[threadIdx.x]);
        if (s_frame[threadIdx.x]) atomicAdd(&a->frame, s_frame[threadIdx.x]);
        atomicMax(&a->key, s_key[threadIdx.x]);
    }
}

// grid (ceil(H W / 256), N): out[p] = the label of a kept pixel, MC_NOT_KEPT elsewhere
__global__ __launch_bounds__(MC_THREADS) void mc_keep_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp, const int* __restrict__ ginfo,
                                                             const McAcc* __restrict__ acc, McModes modes, int HW, int ncls, uint8_t* __restrict__ out) {
    const int q = blockIdx.x * MC_THREADS + threadIdx.x, n = blockIdx.y;
    if (q >= HW) return;
    const size_t img = (size_t)n * HW;
    const int l = labels[img + q];
    bool kept = false;
    if (l < ncls) {
        const int id = comp[img + q], mode = modes.m[l];
        kept = mode == MC_ALL ? true
             : mode == MC_LARGEST ? (0xFFFFFFFFu - (uint32_t)acc[(size_t)n * MC_MAX_CLS + l].key) == (uint32_t)id
                                  : (ginfo[img + id] & MC_FRAME_BIT) != 0;
    }
    out[img + q] = kept ? (uint8_t)l : MC_NOT_KEPT;
}

// ---------------------------------------------------------------------------------------- the fill
// grid (ceil(W / 64), N, ncls), 64 threads: a lane owns one (image, class, column) and walks it down, then up.
// ws[((n H + y) ncls + c) W + x] = the vertical distance to the nearest kept pixel of class c in this column.  The workgroups of the
// first column block also write stats[n][c] = {components, pixels before, pixels removed, pixels kept}; the row pass adds what it fills.
__global__ __launch_bounds__(DIST_COL_THREADS) void mc_fill_col_kernel(const uint8_t* __restrict__ kept, const McAcc* __restrict__ acc, McModes modes, int H, int W,
                                                                       int ncls, uint16_t* __restrict__ ws, int32_t* __restrict__ stats) {
    const int x = blockIdx.x * DIST_COL_THREADS + threadIdx.x, n = blockIdx.y, c = blockIdx.z;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const McAcc a = acc[(size_t)n * MC_MAX_CLS + c];
        const int mode = modes.m[c], stay = mode == MC_ALL ? a.before : mode == MC_LARGEST ? (int)(a.key >> 32) : a.frame;
        int32_t* s = stats + ((size_t)n * ncls + c) * 4;
        s[0] = a.ncomp; s[1] = a.before; s[2] = a.before - stay; s[3] = stay;
    }
    if (x >= W) return;
    const uint8_t* lab = kept + (size_t)n * H * W + x;
    uint16_t* col = ws + ((size_t)n * H * ncls + c) * W + x;
    const size_t pitch = (size_t)ncls * W;
    int in = -1;                                             // the last row seen of the class; -1: none yet
    for (int y0 = 0; y0 < H; y0 += DIST_COL_DEPTH) {
        int l[DIST_COL_DEPTH];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) l[u] = lab[(size_t)min(y0 + u, H - 1) * W];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = y0 + u;
            if (y < H) {
                if (l[u] == c) in = y;
                col[y * pitch] = (uint16_t)dist_to_last(y, in);
            }
        }
    }
    in = -1;                                                 // now the next row below
    for (int y0 = H - 1; y0 >= 0; y0 -= DIST_COL_DEPTH) {
        int l[DIST_COL_DEPTH];
        uint32_t v[DIST_COL_DEPTH];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = max(y0 - u, 0);
            l[u] = lab[(size_t)y * W];
            v[u] = col[y * pitch];
        }
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = y0 - u;
            if (y >= 0) {
                if (l[u] == c) in = y;
                col[y * pitch] = (uint16_t)min(v[u], dist_to_last(y, in));
            }
        }
    }
}

// grid (H, N), W rounded up to whole waves and at most 256 threads.  A row whose pixels are all kept ends at once.  `out` holds the
// kept labels on entry; a pixel that is not kept takes argmin over c of (d^2_c, c), or its own label when the image keeps nothing.
__global__ __launch_bounds__(MC_THREADS) void mc_fill_row_kernel(const uint8_t* __restrict__ labels, const uint16_t* __restrict__ ws, int H, int W, int ncls,
                                                                 uint8_t* out, int32_t* __restrict__ stats) {
    constexpr int PER = DIST_MAX_SIDE / MC_THREADS;          // pixels of a lane at most
    __shared__ u32x4_t s_g[DIST_MAX_SIDE];                   // [x'][j]: g^2 to class c0 + j, DIST_NONE where the column has none
    __shared__ int s_fill[MC_MAX_CLS];
    const int y = blockIdx.x, n = blockIdx.y;
    const size_t row = ((size_t)n * H + y) * W;
    bool mine[PER];
    int any = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int x = k * blockDim.x + threadIdx.x;
        mine[k] = x < W && out[row + x] == MC_NOT_KEPT;
        any |= mine[k];
    }
    if (threadIdx.x < MC_MAX_CLS) s_fill[threadIdx.x] = 0;
    if (!__syncthreads_or(any)) return;
    uint32_t best[PER];
    int cls[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) { best[k] = DIST_NONE; cls[k] = -1; }
    const uint16_t* wrow = ws + row * ncls;
    for (int c0 = 0; c0 < ncls; c0 += 4) {
        if (c0) __syncthreads();
        for (int i = threadIdx.x; i < 4 * W; i += blockDim.x) {
            const int j = i / W, xs = i - j * W;             // consecutive lanes, consecutive x of one class: coalesced
            ((uint32_t*)s_g)[4 * xs + j] = c0 + j < ncls ? dist_sq16(wrow[(size_t)(c0 + j) * W + xs]) : DIST_NONE;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!mine[k]) continue;
            const int x = k * blockDim.x + threadIdx.x;
            uint32_t m[4] = {DIST_NONE, DIST_NONE, DIST_NONE, DIST_NONE};
            for (int xs = 0; xs < W; ++xs) {
                const uint32_t dx = (uint32_t)((x - xs) * (x - xs));
                const u32x4_t g = s_g[xs];
                m[0] = min(m[0], dx + g[0]);
                m[1] = min(m[1], dx + g[1]);
                m[2] = min(m[2], dx + g[2]);
                m[3] = min(m[3], dx + g[3]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (m[j] < best[k]) { best[k] = m[j]; cls[k] = c0 + j; }     // strictly less, classes ascending: a tie stays with the lower class
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!mine[k]) continue;
        const int x = k * blockDim.x + threadIdx.x;
        out[row + x] = cls[k] >= 0 ? (uint8_t)cls[k] : labels[row + x];
        if (cls[k] >= 0) atomicAdd(&s_fill[cls[k]], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < ncls && s_fill[threadIdx.x]) atomicAdd(&stats[((size_t)n * ncls + threadIdx.x) * 4 + 3], s_fill[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------- launchers
// the checks of the shape, in the order the header states
int mc_check(const char* name, int N, int H, int W, int ncls, int conn, const uint8_t* modes) {
    if (N < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: N=%d H=%d W=%d (every size must be at least 1)", name, N, H, W);
    if (conn != 4 && conn != 8) S2E_FAIL(S2E_ERR_ARG, "%s: conn=%d (4 or 8)", name, conn);
    if (ncls < 1 || ncls > MC_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: ncls=%d (1 to %d classes)", name, ncls, MC_MAX_CLS);
    for (int c = 0; modes && c < ncls; ++c)
        if (modes[c] > MC_FRAME) S2E_FAIL(S2E_ERR_ARG, "%s: modes[%d]=%d (0 all, 1 largest, 2 border)", name, c, (int)modes[c]);
    if (H > DIST_MAX_SIDE || W > DIST_MAX_SIDE) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (each at most %d)", name, H, W, DIST_MAX_SIDE);
    return s2e_check_image_batch(name, N, H, W);
}

bool mc_shape_ok(int N, int H, int W, int ncls) {
    return N >= 1 && H >= 1 && W >= 1 && ncls >= 1 && ncls <= MC_MAX_CLS && H <= DIST_MAX_SIDE && W <= DIST_MAX_SIDE && N <= 65535 &&
           (long)N * H * W < (1L << 31);
}

// the sections of s2e_mask_clean's workspace, each starting on 256 bytes
struct McPlan { size_t comp, tinfo, ginfo, acc, stats, dist, total; };
McPlan mc_plan(int N, int H, int W, int ncls) {
    const size_t P = (size_t)N * H * W;
    McPlan p;
    size_t at = 0;
    p.comp = at;  at += s2e_align256(P * sizeof(int));
    p.tinfo = at; at += s2e_align256(P * sizeof(int));
    p.ginfo = at; at += s2e_align256(P * sizeof(int));
    p.acc = at;   at += s2e_align256((size_t)N * MC_MAX_CLS * sizeof(McAcc));
    p.stats = at; at += s2e_align256((size_t)N * ncls * 4 * sizeof(int32_t));
    p.dist = at;  at += s2e_align256(P * ncls * sizeof(uint16_t));
    p.total = at;
    return p;
}

// label, merge, flatten on `parent`
template <bool INFO>
int mc_components(const uint8_t* labels, int N, int H, int W, int ncls, int conn, int* parent, int* tinfo, int* ginfo, McAcc* acc, hipStream_t st) {
    mc_label_kernel<INFO><<<dim3(ceil_div(W, MC_TILE), ceil_div(H, MC_TILE), N), MC_THREADS, 0, st>>>(labels, H, W, ncls, conn, parent, tinfo, ginfo, acc);
    S2E_CHECK_LAUNCH("mc_label_kernel");
    if (H > MC_TILE || W > MC_TILE) {                                    // (one tile per image: nothing to join)
        mc_merge_kernel<<<dim3(ceil_div(W, MC_THREADS), H, N), MC_THREADS, 0, st>>>(labels, H, W, ncls, conn, parent);
        S2E_CHECK_LAUNCH("mc_merge_kernel");
    }
    mc_flatten_kernel<INFO><<<dim3(ceil_div((long)H * W, MC_THREADS), N), MC_THREADS, 0, st>>>(H * W, parent, tinfo, ginfo);
    S2E_CHECK_LAUNCH("mc_flatten_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_mask_clean_workspace_bytes(int N, int H, int W, int ncls) {
    return mc_shape_ok(N, H, W, ncls) ? mc_plan(N, H, W, ncls).total : 0;
}

extern "C" int s2e_mask_components(const uint8_t* labels, int N, int H, int W, int ncls, int conn, int32_t* comp, void* stream) {
    const char* name = "s2e_mask_components";
    if (!labels || !comp) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (const int rc = mc_check(name, N, H, W, ncls, conn, nullptr)) return rc;
    return mc_components<false>(labels, N, H, W, ncls, conn, comp, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int s2e_mask_clean(const uint8_t* labels, int N, int H, int W, int ncls, int conn, const uint8_t* modes, uint8_t* out, int32_t* stats,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "s2e_mask_clean";
    if (!labels || !out || !modes || !workspace) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    const size_t need = s2e_mask_clean_workspace_bytes(N, H, W, ncls);   // (0 for a shape the checks below refuse)
    if (workspace_bytes < need || ((uintptr_t)workspace & 7))
        S2E_FAIL(S2E_ERR_ARG, "%s: workspace of %zu bytes, needs %zu (8-byte aligned)", name, workspace_bytes, need);
    if (const int rc = mc_check(name, N, H, W, ncls, conn, modes)) return rc;
    const McPlan plan = mc_plan(N, H, W, ncls);
    char* ws = (char*)workspace;
    int* comp = (int*)(ws + plan.comp);
    int* tinfo = (int*)(ws + plan.tinfo);
    int* ginfo = (int*)(ws + plan.ginfo);
    McAcc* acc = (McAcc*)(ws + plan.acc);
    uint16_t* dist = (uint16_t*)(ws + plan.dist);
    if (!stats) stats = (int32_t*)(ws + plan.stats);
    McModes mm{};
    for (int c = 0; c < ncls; ++c) mm.m[c] = modes[c];
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    if (const int rc = mc_components<true>(labels, N, H, W, ncls, conn, comp, tinfo, ginfo, acc, st)) return rc;
    const int blocks = ceil_div(HW, MC_THREADS);
    mc_best_kernel<<<dim3(blocks < MC_BEST_BLOCKS ? blocks : MC_BEST_BLOCKS, N), MC_THREADS, 0, st>>>(labels, comp, ginfo, HW, ncls, acc);
    S2E_CHECK_LAUNCH("mc_best_kernel");
    mc_keep_kernel<<<dim3(blocks, N), MC_THREADS, 0, st>>>(labels, comp, ginfo, acc, mm, HW, ncls, out);
    S2E_CHECK_LAUNCH("mc_keep_kernel");
    mc_fill_col_kernel<<<dim3(ceil_div(W, DIST_COL_THREADS), N, ncls), DIST_COL_THREADS, 0, st>>>(out, acc, mm, H, W, ncls, dist, stats);
    S2E_CHECK_LAUNCH("mc_fill_col_kernel");
    mc_fill_row_kernel<<<dim3(H, N), dist_row_threads(W, MC_THREADS), 0, st>>>(labels, dist, H, W, ncls, out, stats);
    S2E_CHECK_LAUNCH("mc_fill_row_kernel");
    return S2E_OK;
}
