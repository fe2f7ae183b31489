// LiDAR depth association of the feature tracker (include/lvi_depth.h): the reference's lidar_callback
// (feature_tracker_node.cpp:273-377) and DepthRegister::get_depth (feature_tracker.h:116-331) on one stream.
//
// Cloud side, per used cloud:  H2D -> VoxelGrid 0.2 (the general voxel path, lvi_voxel.hpp) -> field-of-view cut +
// getTransformation (two kernels: per-block counts, then an ordered write into a slot of the device ring) -> the
// window's slots concatenated in queue order -> VoxelGrid 0.2 = the depth cloud.  The queue itself (slots, stamps, the
// 5 s pop) is host state.
// Frame side, per get_depth:  range image = 360x360 u64 keys (dist bits << 32 | cloud index) filled by atomicMin ->
// per-row counts -> ordered compaction onto the unit sphere (row-major) -> one workgroup per feature: exact 3-NN over
// the rows of a band around the feature's row, plane intersection, depth.  Results go to pinned memory, one wait.
// Every f32 operation is written in the reference's order; the library is built with -ffp-contract=off.
#include <cmath>
#include <cfloat>
#include <deque>

#include "../../include/lvi_depth.h"
#include "lvi_voxel.hpp"

using namespace lvi;

namespace {

constexpr int NB = LVI_DEPTH_BINS;                 // num_bins
constexpr int NBINS = NB * NB;
constexpr float BIN_RES = 180.0f / (float)NB;      // float bin_res = 180.0 / (float)num_bins
constexpr int FOV_BLOCK = 1024;                    // points per workgroup of the field-of-view compaction
constexpr int ROW_THREADS = 384;                   // >= NB: one thread per bin of a row
constexpr int KNN_THREADS = 256;
// Band of the 3-NN search.  The reference accepts only when its 3rd neighbour lies at a squared chord below
// dist_sq_threshold = (5 sin(0.5 deg))^2, i.e. within 2 asin(2.5 sin 0.5 deg) = 2.4998 deg of arc of the feature's ray; so
// do all three neighbours.  A sphere point's row is round(elevation / 0.5 deg) of its own elevation, which differs from
// the feature's by at most that arc: |row - feature_row_real| <= 2.4998 / 0.5 + 0.5 (rounding) = 5.5 rows.  Searching
// the rows within 7 of the feature's real-valued row (1.5 rows of slack for f32 error in the angles) holds every point
// the reference could accept, so the band's 3-NN equals the unrestricted 3-NN whenever the reference accepts, and when it
// rejects the band's 3rd distance is no smaller than the true one: rejected as well.
constexpr int BAND_ROWS = 7;
constexpr double DEG_PER_RAD = 180.0 / M_PI;

struct Mat34 { float m[12]; };                     // row-major 3x4 affine

// pcl::getTransformation(x, y, z, roll, pitch, yaw), f32, host libm (as lvo::getTransformation and kf_matrix)
Mat34 get_transformation(const float p[6])
{
    const float A = std::cos(p[5]), B = std::sin(p[5]), C = std::cos(p[4]), D = std::sin(p[4]), E = std::cos(p[3]), F = std::sin(p[3]);
    const float DE = D * E, DF = D * F;
    return Mat34{{A * C, A * DF - B * E, B * F + A * DE, p[0],  B * C, A * E + B * DF, B * DE - A * F, p[1],  -D, C * F, C * E, p[2]}};
}

// Eigen::Affine3f::inverse(): linear part by the 3x3 cofactor inverse (InverseImpl.h: cofactor_3x3, det = c0 . col0
// reduced as a0 + (a1 + a2), inv(i,j) = cofactor(j,i) * invdet), then translation = -(inv * t), each row reduced as above
Mat34 affine_inverse(const Mat34& T)
{
    auto m = [&](int r, int c) { return T.m[4 * r + c]; };
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m(i1, j1) * m(i2, j2) - m(i1, j2) * m(i2, j1);
    };
    const float c0[3] = {cof(0, 0), cof(1, 0), cof(2, 0)};
    const float det = c0[0] * m(0, 0) + (c0[1] * m(1, 0) + c0[2] * m(2, 0));
    const float invdet = 1.0f / det;
    Mat34 R;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R.m[4 * i + j] = cof(j, i) * invdet;
    for (int i = 0; i < 3; i++) {
        const float* r = &R.m[4 * i];
        R.m[4 * i + 3] = -(r[0] * m(0, 3) + (r[1] * m(1, 3) + r[2] * m(2, 3)));
    }
    return R;
}

__device__ __forceinline__ lvi_pt affine(const Mat34& M, const lvi_pt& p)     // pcl::transformPointCloud (the library's to_map order)
{
    lvi_pt o;
    o.x = M.m[0] * p.x + M.m[1] * p.y + M.m[2] * p.z + M.m[3];
    o.y = M.m[4] * p.x + M.m[5] * p.y + M.m[6] * p.z + M.m[7];
    o.z = M.m[8] * p.x + M.m[9] * p.y + M.m[10] * p.z + M.m[11];
    o.intensity = p.intensity;
    return o;
}

__device__ __forceinline__ bool fov_keep(const lvi_pt& p)        // lidar_callback step 3
{
    return p.x >= 0.f && fabsf(p.y / p.x) <= 10.f && fabsf(p.z / p.x) <= 10.f;
}
__device__ __forceinline__ float point_distance(const lvi_pt& p) { return sqrtf(p.x * p.x + p.y * p.y + p.z * p.z); }

// ---------------------------------------------------------------------------------------------- cloud side
__global__ __launch_bounds__(FOV_BLOCK) void fov_count_kernel(const lvi_pt* in, const int* d_n, int* blk_cnt)
{
    const int n = *d_n, i = blockIdx.x * FOV_BLOCK + threadIdx.x;
    const int keep = (i < n && fov_keep(ld_global_pt(in + i))) ? 1 : 0;
    __shared__ int ws[FOV_BLOCK / 64 + 1];
    int total = 0;
    block_excl_scan<FOV_BLOCK>(keep, ws, &total);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// the kept points, transformed into the world frame, in input order: offset of the block = sum of the counts before it
__global__ __launch_bounds__(FOV_BLOCK) void fov_write_kernel(const lvi_pt* in, const int* d_n, const int* blk_cnt, Mat34 M, lvi_pt* out, int* d_out_n)
{
    const int n = *d_n, i = blockIdx.x * FOV_BLOCK + threadIdx.x;
    __shared__ int ws[FOV_BLOCK / 64 + 1];
    __shared__ int base;
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += FOV_BLOCK) part += blk_cnt[b];
    int tot = 0;
    block_excl_scan<FOV_BLOCK>(part, ws, &tot);
    if (threadIdx.x == 0) base = tot;
    __syncthreads();
    lvi_pt p{0.f, 0.f, 0.f, 0.f};
    int keep = 0;
    if (i < n) { p = ld_global_pt(in + i); keep = fov_keep(p) ? 1 : 0; }
    int cnt = 0;
    const int pre = block_excl_scan<FOV_BLOCK>(keep, ws, &cnt);
    if (keep) out[base + pre] = affine(M, p);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *d_out_n = base + cnt;
}

struct ConcatArgs { int nq; int slot[LVI_DEPTH_MAX_CLOUDS]; };
// the window's clouds concatenated in queue order (depthCloud += cloudQueue[i]); blockIdx.y = queue position
__global__ __launch_bounds__(256) void concat_kernel(ConcatArgs a, const lvi_pt* ring, const int* ring_n, int cap, lvi_pt* out, int* d_total)
{
    const int q = blockIdx.y;
    int off = 0;
    for (int k = 0; k < q; k++) off += ring_n[a.slot[k]];
    const int s = a.slot[q], n = ring_n[s];
    const lvi_pt* src = ring + (size_t)s * cap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[off + i] = ld_global_pt(src + i);
    if (q == a.nq - 1 && blockIdx.x == 0 && threadIdx.x == 0) *d_total = off + n;
}

// ---------------------------------------------------------------------------------------------- frame side
// get_depth step 3: the closest point per bin; the key's low word (cloud index) makes the lowest index win ties, which is
// the strict '<' of the reference's cloud-order loop.  dist >= 0, so its bits order like its value.
__global__ __launch_bounds__(256) void range_image_kernel(const lvi_pt* cloud, const int* d_n, Mat34 Minv, unsigned long long* range)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *d_n) return;
    const lvi_pt p = affine(Minv, ld_global_pt(cloud + i));
    if (p.x < 0.f || fabsf(p.y / p.x) > 10.f || fabsf(p.z / p.x) > 10.f) return;     // NaN ratios (x = y = 0) do not skip
    // atan2(float, float) is atan2f; the device's own atan2f is not correctly rounded, the double one rounded to f32 is
    // (but for double-rounding cases), as glibc's atan2f.  * 180.0 / M_PI + 90.0 in double, stored as float.
    const float ra = (float)atan2((double)p.z, (double)sqrtf(p.x * p.x + p.y * p.y));
    const float row_angle = (float)((double)ra * 180.0 / M_PI + 90.0);
    const int row_id = (int)roundf(row_angle / BIN_RES);
    const float ca = (float)atan2((double)p.x, (double)p.y);
    const float col_angle = (float)((double)ca * 180.0 / M_PI);
    const int col_id = (int)roundf(col_angle / BIN_RES);
    if (row_id < 0 || row_id >= NB || col_id < 0 || col_id >= NB) return;
    const float dist = point_distance(p);
    if (!(dist < FLT_MAX)) return;                                                       // rangeImage starts at FLT_MAX
    atomicMin(range + row_id * NB + col_id, ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)i);
}

__global__ __launch_bounds__(ROW_THREADS) void row_count_kernel(const unsigned long long* range, int* row_n)
{
    const int r = blockIdx.x, c = threadIdx.x;
    const int occ = (c < NB && range[r * NB + c] != ~0ull) ? 1 : 0;
    __shared__ int ws[ROW_THREADS / 64 + 1];
    int total = 0;
    block_excl_scan<ROW_THREADS>(occ, ws, &total);
    if (c == 0) row_n[r] = total;
}

// steps 4-5: the occupied bins in row-major order, projected onto the unit sphere (intensity = range); row_off[NB + 1]
__global__ __launch_bounds__(ROW_THREADS) void sphere_kernel(const unsigned long long* range, const int* row_n, const lvi_pt* cloud, Mat34 Minv,
                                                             lvi_pt* sphere, int* row_off, int* d_nsph)
{
    const int r = blockIdx.x, c = threadIdx.x;
    __shared__ int ws[ROW_THREADS / 64 + 1];
    int part = 0;
    for (int k = c; k < r; k += ROW_THREADS) part += row_n[k];
    int base = 0;
    block_excl_scan<ROW_THREADS>(part, ws, &base);
    const unsigned long long key = c < NB ? range[r * NB + c] : ~0ull;
    const int occ = key != ~0ull ? 1 : 0;
    int cnt = 0;
    const int pre = block_excl_scan<ROW_THREADS>(occ, ws, &cnt);
    if (occ) {
        lvi_pt p = affine(Minv, ld_global_pt(cloud + (unsigned)key));
        const float rng = point_distance(p);
        p.x /= rng; p.y /= rng; p.z /= rng; p.intensity = rng;
        sphere[base + pre] = p;
    }
    if (c == 0) row_off[r] = base;
    if (r == NB - 1 && c == 0) { row_off[NB] = base + cnt; *d_nsph = base + cnt; }
}

__device__ __forceinline__ void top3_insert(unsigned long long k, unsigned long long t[3])
{
    if (k < t[2]) {
        if (k < t[1]) { t[2] = t[1]; if (k < t[0]) { t[1] = t[0]; t[0] = k; } else t[1] = k; }
        else t[2] = k;
    }
}

// steps 6-7 and the depth channel: one workgroup per feature.  Neighbour keys = (sqd bits << 32 | sphere index): exact,
// sorted by distance, lower index first on ties.  NaN distances (the origin's sphere image) never enter.
__global__ __launch_bounds__(KNN_THREADS) void knn_depth_kernel(const float* feat, int nf, const lvi_pt* sphere, const int* row_off, const int* d_nsph,
                                                                float thr, int full, float* depth, int* nbr, float* nsqd)
{
    const int f = blockIdx.x;
    if (f >= nf) return;
    // 0.5: Eigen normalize() (squaredNorm reduced as a0 + (a1 + a2), then /= sqrt), ROS axes (z, -x, -y)
    const float fx = feat[3 * f], fy = feat[3 * f + 1], fz = feat[3 * f + 2];
    const float sq = fx * fx + (fy * fy + fz * fz);
    float nx = fx, ny = fy, nz = fz;
    if (sq > 0.f) { const float s = sqrtf(sq); nx = fx / s; ny = fy / s; nz = fz / s; }
    const float vx = nz, vy = -nx, vz = -ny;
    const int nsph = *d_nsph;
    if (nsph < 10) {
        if (threadIdx.x == 0) { depth[f] = -1.f; for (int k = 0; k < 3; k++) { nbr[3 * f + k] = -1; nsqd[3 * f + k] = -1.f; } }
        return;
    }
    int lo = 0, hi = NB - 1;
    if (!full) {
        const double fr = (atan2((double)vz, sqrt((double)vx * vx + (double)vy * vy)) * DEG_PER_RAD + 90.0) / (double)BIN_RES;
        if (fr == fr) { lo = max(0, (int)floor(fr - BAND_ROWS)); hi = min(NB - 1, (int)ceil(fr + BAND_ROWS)); }     // (a zero feature: every row)
    }
    unsigned long long t[3] = {~0ull, ~0ull, ~0ull};
    if (lo <= hi) {
        const int b = row_off[lo], e = row_off[hi + 1];
        for (int j = b + threadIdx.x; j < e; j += KNN_THREADS) {
            const lvi_pt p = ld_global_pt(sphere + j);
            const float dx = vx - p.x, dy = vy - p.y, dz = vz - p.z;
            const float d = dx * dx + dy * dy + dz * dz;                                   // FLANN's L2_Simple order
            if (d == d) top3_insert(((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j, t);
        }
    }
    // workgroup top-3: three rounds of a u64 min over the 3 * 256 candidates
    __shared__ unsigned long long cand[3 * KNN_THREADS];
    __shared__ unsigned long long wmin[KNN_THREADS / 64];
    __shared__ unsigned long long best[3];
    for (int k = 0; k < 3; k++) cand[3 * threadIdx.x + k] = t[k];
    __syncthreads();
    for (int round = 0; round < 3; round++) {
        unsigned long long m = ~0ull;
        for (int k = 0; k < 3; k++) m = min(m, cand[3 * threadIdx.x + k]);
        for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, o, 64));
        if (lane_id() == 0) wmin[wave_id()] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long g = wmin[0];
            for (int w = 1; w < KNN_THREADS / 64; w++) g = min(g, wmin[w]);
            best[round] = g;
        }
        __syncthreads();
        const unsigned long long g = best[round];
        if (g != ~0ull)
            for (int k = 0; k < 3; k++) if (cand[3 * threadIdx.x + k] == g) cand[3 * threadIdx.x + k] = ~0ull;     // keys are unique (index)
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float out = -1.f;
    for (int k = 0; k < 3; k++) {
        nbr[3 * f + k] = best[k] == ~0ull ? -1 : (int)(unsigned)best[k];
        nsqd[3 * f + k] = best[k] == ~0ull ? -1.f : __uint_as_float((unsigned)(best[k] >> 32));
    }
    if (best[2] != ~0ull && __uint_as_float((unsigned)(best[2] >> 32)) < thr) {
        const lvi_pt P1 = sphere[(unsigned)best[0]], P2 = sphere[(unsigned)best[1]], P3 = sphere[(unsigned)best[2]];
        const float r1 = P1.intensity, r2 = P2.intensity, r3 = P3.intensity;
        const float Ax = P1.x * r1, Ay = P1.y * r1, Az = P1.z * r1;
        const float Bx = P2.x * r2, By = P2.y * r2, Bz = P2.z * r2;
        const float Cx = P3.x * r3, Cy = P3.y * r3, Cz = P3.z * r3;
        const float ux = Ax - Bx, uy = Ay - By, uz = Az - Bz;          // A - B
        const float wx = Bx - Cx, wy = By - Cy, wz = Bz - Cz;          // B - C
        const float Nx = uy * wz - uz * wy, Ny = uz * wx - ux * wz, Nz = ux * wy - uy * wx;   // Eigen cross
        float s = (Nx * Ax + Ny * Ay + Nz * Az) / (Nx * vx + Ny * vy + Nz * vz);
        const float min_depth = fminf(r1, fminf(r2, r3)), max_depth = fmaxf(r1, fmaxf(r2, r3));
        if (!(max_depth - min_depth > 2.f || s <= 0.5f)) {
            if (s - max_depth > 0.f) s = max_depth;
            else if (s - min_depth < 0.f) s = min_depth;
            const float d = vx * s;                                    // intensity = x * s
            if ((double)d > 3.0) out = d;
        }
    }
    depth[f] = out;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_depth : Handle {
    int C = 0, P = 0, F = 0, skip = 0;
    double window = 5.0;
    Ctx ctx;                               // ctx.stream is the handle's stream
    VoxelPlan vox1, vox2;
    lvi_pt *rawIn = nullptr, *vOut = nullptr, *ring = nullptr, *fused = nullptr, *cloud = nullptr, *sphere = nullptr;
    int *ringN = nullptr, *blkCnt = nullptr, *fusedN = nullptr, *cloudN = nullptr, *rowN = nullptr, *rowOff = nullptr, *nsph = nullptr, *nbr = nullptr;
    unsigned long long* range = nullptr;
    float *feat = nullptr, *depth = nullptr, *nsqd = nullptr;
    float* h_io = nullptr;                 // pinned: features in, depths out
    int* h_cnt = nullptr;                  // pinned [16]: [0] depth cloud size
    // host state of the window
    int lidar_count = -1, used_total = 0, cloud_n = 0, fused_n_last = 0;
    std::deque<int> slots;
    std::deque<double> stamps;
    int last_nf = 0;
    bool searched = false, full = false;
    float thr = 0.f;
};

namespace {

template <class AR, class PIN> void depth_layout(AR& ar, PIN& pin, lvi_depth& h)
{
    const size_t W = (size_t)h.C * h.P;
    h.h_io = pin.template alloc<float>((size_t)3 * h.F); h.h_cnt = pin.template alloc<int>(16);
    h.rawIn = ar.template alloc<lvi_pt>(h.P); h.vOut = ar.template alloc<lvi_pt>(h.P);
    h.ring = ar.template alloc<lvi_pt>(W); h.ringN = ar.template alloc<int>(h.C);
    h.blkCnt = ar.template alloc<int>(div_up(h.P, FOV_BLOCK));
    h.fused = ar.template alloc<lvi_pt>(W); h.fusedN = ar.template alloc<int>(1);
    h.cloud = ar.template alloc<lvi_pt>(W); h.cloudN = ar.template alloc<int>(1);
    h.range = ar.template alloc<unsigned long long>(NBINS);
    h.rowN = ar.template alloc<int>(NB); h.rowOff = ar.template alloc<int>(NB + 1); h.nsph = ar.template alloc<int>(1);
    h.sphere = ar.template alloc<lvi_pt>(NBINS);
    h.feat = ar.template alloc<float>((size_t)3 * h.F); h.depth = ar.template alloc<float>(h.F);
    h.nbr = ar.template alloc<int>((size_t)3 * h.F); h.nsqd = ar.template alloc<float>((size_t)3 * h.F);
    h.vox1.allocate(ar, 1, h.P, false);
    h.vox2.allocate(ar, 1, (int)W, false);
}

void wait(lvi_depth* h) { LVI_HIP(hipStreamSynchronize(h->ctx.stream)); }

// steps 2-9 of lidar_callback for a cloud already in rawIn
int32_t cloud_enqueue(lvi_depth* h, int n, const float pose6[6], double stamp, int32_t* used)
{
    const Ctx& c = h->ctx;
    // 7 first (it only depends on the new stamp): the window must have a free slot for the new cloud
    size_t pops = 0;
    while (pops < h->stamps.size() && stamp - h->stamps[pops] > h->window) pops++;
    if (h->slots.size() - pops + 1 > (size_t)h->C) return fail(LVI_ERR_CAPACITY, "the window would hold more than max_clouds clouds");
    // 2. VoxelGrid 0.2 of the raw cloud
    h->vox1.n_host[0] = n; h->vox1.use_n_host = true;
    voxel_downsample_batch(c, h->vox1, "depth_vox_in", n);
    // 3 + 5. field of view, world frame, into a free ring slot
    std::vector<bool> busy(h->C, false);
    for (int s : h->slots) busy[s] = true;
    for (size_t k = 0; k < pops; k++) busy[h->slots[k]] = false;
    int slot = 0;
    while (busy[slot]) slot++;
    const Mat34 M = get_transformation(pose6);
    const int nblk = div_up(std::max(h->P, 1), FOV_BLOCK);
    LVI_LAUNCH(c, "depth_fov_count", 16.0 * n, hipLaunchKernelGGL(fov_count_kernel, dim3(nblk), dim3(FOV_BLOCK), 0, c.stream, h->vOut, h->vox1.d_nout, h->blkCnt));
    LVI_LAUNCH(c, "depth_fov_write", 32.0 * n, hipLaunchKernelGGL(fov_write_kernel, dim3(nblk), dim3(FOV_BLOCK), 0, c.stream, h->vOut, h->vox1.d_nout, h->blkCnt, M,
                                                                  h->ring + (size_t)slot * h->P, h->ringN + slot));
    // 6-7. push, pop
    for (size_t k = 0; k < pops; k++) { h->slots.pop_front(); h->stamps.pop_front(); }
    h->slots.push_back(slot); h->stamps.push_back(stamp);
    // 8-9. fuse in queue order, VoxelGrid 0.2
    ConcatArgs a{};
    a.nq = (int)h->slots.size();
    for (int q = 0; q < a.nq; q++) a.slot[q] = h->slots[q];
    LVI_LAUNCH(c, "depth_concat", 32.0 * h->P * a.nq, hipLaunchKernelGGL(concat_kernel, dim3(div_up(h->P, 256 * 4), a.nq), dim3(256), 0, c.stream, a, h->ring, h->ringN,
                                                                          h->P, h->fused, h->fusedN));
    h->vox2.last_mode = voxel_downsample_batch(c, h->vox2, "depth_vox_window", (double)h->P * a.nq).mode;
    LVI_HIP(hipMemcpyAsync(h->cloudN, h->vox2.d_nout, sizeof(int), hipMemcpyDeviceToDevice, c.stream));
    LVI_HIP(hipMemcpyAsync(h->h_cnt, h->vox2.d_nout, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    LVI_HIP(hipMemcpyAsync(h->h_cnt + 1, h->fusedN, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    wait(h);
    h->cloud_n = h->h_cnt[0]; h->fused_n_last = h->h_cnt[1];
    h->used_total++;
    if (used) *used = 1;
    return LVI_OK;
}

int32_t cloud_entry(lvi_depth* h, const lvi_pt* pts, bool device, int32_t n, const float pose6[6], double stamp, int32_t* used)
{
    if (!h || n < 0 || (n > 0 && !pts)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if (n > h->P) return fail(LVI_ERR_CAPACITY, "n exceeds max_cloud_points");
    if (used) *used = 0;
    if (++h->lidar_count % (h->skip + 1) != 0) return LVI_OK;        // static int lidar_count = -1; ++ % (LIDAR_SKIP + 1)
    if (!pose6) return LVI_OK;                                        // no TF: nothing else changes
    return guarded(h->device, [&]() -> int32_t {
        if (n > 0) LVI_HIP(hipMemcpyAsync(h->rawIn, pts, sizeof(lvi_pt) * (size_t)n, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->ctx.stream));
        return cloud_enqueue(h, n, pose6, stamp, used);
    });
}

}  // namespace

extern "C" {

int32_t lvi_depth_abi_version(void) { return LVI_DEPTH_ABI_VERSION; }

int32_t lvi_depth_create(int32_t device, int32_t max_clouds, int32_t max_cloud_points, int32_t max_features, int32_t lidar_skip, double window_s, lvi_depth** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_clouds < 1 || max_clouds > LVI_DEPTH_MAX_CLOUDS) return fail(LVI_ERR_INVALID_ARG, "max_clouds must be 1..LVI_DEPTH_MAX_CLOUDS");
    if (max_cloud_points < 1 || max_features < 1 || lidar_skip < 0 || !(window_s >= 0.0)) return fail(LVI_ERR_INVALID_ARG, "bad capacities");
    if ((long long)max_clouds * max_cloud_points > (1 << 25) || max_features > (1 << 20)) return fail(LVI_ERR_INVALID_ARG, "capacities above 2^25 window points are not supported");
    return create_handle(device, out, lvi_depth_destroy, [&](lvi_depth* h) {
        h->C = max_clouds; h->P = max_cloud_points; h->F = max_features; h->skip = lidar_skip; h->window = window_s;
        // float dist_sq_threshold = pow(sin(bin_res / 180.0 * M_PI) * 5.0, 2)
        h->thr = (float)std::pow(std::sin((double)BIN_RES / 180.0 * M_PI) * 5.0, 2);
    }, [&](lvi_depth* h) -> int32_t {
        h->open(device, [&](auto& dev, auto& pin) { depth_layout(dev, pin, *h); }, 1 << 16);
        h->ctx.stream = h->stream;
        VoxSegStatic s1{h->rawIn, nullptr, h->vOut, 0.2f}, s2{h->fused, nullptr, h->cloud, 0.2f};
        h->vox1.set_static(h->ctx, &s1);
        h->vox2.set_static(h->ctx, &s2);
        h->vox2.n_dev[0] = h->fusedN;
        LVI_HIP(hipMemsetAsync(h->cloudN, 0, sizeof(int), h->ctx.stream));
        LVI_HIP(hipMemsetAsync(h->fusedN, 0, sizeof(int), h->ctx.stream));
        wait(h);
        return LVI_OK;
    });
}

void lvi_depth_destroy(lvi_depth* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->vox1.release(); h->vox2.release();                       // before the arena goes
    h->close();
    delete h;
}

int32_t lvi_depth_lidar_cloud(lvi_depth* h, const lvi_pt* pts, int32_t n, const float pose6[6], double stamp, int32_t* used)
{
    return cloud_entry(h, pts, false, n, pose6, stamp, used);
}
int32_t lvi_depth_lidar_cloud_device(lvi_depth* h, const lvi_pt* d_pts, int32_t n, const float pose6[6], double stamp, int32_t* used)
{
    return cloud_entry(h, d_pts, true, n, pose6, stamp, used);
}

int32_t lvi_depth_get(lvi_depth* h, const float pose6[6], const float* features_xyz, int32_t n, float* depth_out)
{
    if (!h || n < 0 || (n > 0 && (!features_xyz || !depth_out))) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if (n > h->F) return fail(LVI_ERR_CAPACITY, "n exceeds max_features");
    for (int i = 0; i < n; i++) depth_out[i] = -1.f;                  // depth_of_point.values.resize(n, -1)
    // 0.2 / 0.3: no depth cloud or no transform: the initial values, the GPU state is not touched
    if (!pose6) return LVI_OK;                                        // (the debug views keep the previous call's)
    if (h->cloud_n == 0 || n == 0) { h->searched = false; h->last_nf = 0; return LVI_OK; }
    return guarded(h->device, [&]() -> int32_t {
        const Ctx& c = h->ctx;
        const Mat34 Minv = affine_inverse(get_transformation(pose6));
        std::memcpy(h->h_io, features_xyz, sizeof(float) * 3 * (size_t)n);
        LVI_HIP(hipMemcpyAsync(h->feat, h->h_io, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c.stream));
        LVI_HIP(hipMemsetAsync(h->range, 0xff, sizeof(unsigned long long) * NBINS, c.stream));
        const int W = h->cloud_n;
        LVI_LAUNCH(c, "depth_range_image", 32.0 * W, hipLaunchKernelGGL(range_image_kernel, dim3(div_up(W, 256)), dim3(256), 0, c.stream, h->cloud, h->cloudN, Minv, h->range));
        LVI_LAUNCH(c, "depth_row_count", 8.0 * NBINS, hipLaunchKernelGGL(row_count_kernel, dim3(NB), dim3(ROW_THREADS), 0, c.stream, h->range, h->rowN));
        LVI_LAUNCH(c, "depth_sphere", 8.0 * NBINS, hipLaunchKernelGGL(sphere_kernel, dim3(NB), dim3(ROW_THREADS), 0, c.stream, h->range, h->rowN, h->cloud, Minv,
                                                                      h->sphere, h->rowOff, h->nsph));
        LVI_LAUNCH(c, "depth_knn", 16.0 * n, hipLaunchKernelGGL(knn_depth_kernel, dim3(n), dim3(KNN_THREADS), 0, c.stream, h->feat, n, h->sphere, h->rowOff, h->nsph,
                                                                h->thr, h->full ? 1 : 0, h->depth, h->nbr, h->nsqd));
        LVI_HIP(hipMemcpyAsync(h->h_io, h->depth, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c.stream));
        wait(h);
        std::memcpy(depth_out, h->h_io, sizeof(float) * (size_t)n);
        h->searched = true; h->last_nf = n;
        return LVI_OK;
    });
}

int32_t lvi_depth_state(lvi_depth* h, int32_t state[4])
{
    if (!h || !state) return fail(LVI_ERR_INVALID_ARG, "null argument");
    state[0] = (int32_t)h->slots.size(); state[1] = h->lidar_count; state[2] = h->cloud_n; state[3] = h->used_total;
    return LVI_OK;
}

int32_t lvi_depth_set_cloud(lvi_depth* h, const lvi_pt* pts, int32_t n)
{
    if (!h || n < 0 || (n > 0 && !pts)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if ((long long)n > (long long)h->C * h->P) return fail(LVI_ERR_CAPACITY, "n exceeds max_clouds * max_cloud_points");
    return guarded(h->device, [&]() -> int32_t {
        if (n > 0) LVI_HIP(hipMemcpyAsync(h->cloud, pts, sizeof(lvi_pt) * (size_t)n, hipMemcpyHostToDevice, h->ctx.stream));
        h->h_cnt[2] = n;
        LVI_HIP(hipMemcpyAsync(h->cloudN, h->h_cnt + 2, sizeof(int), hipMemcpyHostToDevice, h->ctx.stream));
        wait(h);
        h->cloud_n = n;
        return LVI_OK;
    });
}

int32_t lvi_depth_get_cloud(lvi_depth* h, lvi_pt* out, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out || (cap > 0 && !out)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    *n_out = h->cloud_n;
    const int m = std::min(cap, h->cloud_n);
    if (m <= 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        LVI_HIP(hipMemcpyAsync(out, h->cloud, sizeof(lvi_pt) * (size_t)m, hipMemcpyDeviceToHost, h->ctx.stream));
        wait(h);
        return LVI_OK;
    });
}

int32_t lvi_depth_debug_voxel(lvi_depth* h, int32_t* cells, int32_t* counts, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->used_total == 0) return fail(LVI_ERR_STATE, "no window fusion yet");
    return guarded(h->device, [&]() -> int32_t {
        std::vector<int32_t> k, cl, ct;
        voxel_debug_fetch(h->ctx, h->vox2, h->fused_n_last, k, cl, ct);
        *n_out = (int32_t)cl.size();
        const int m = std::min<int>(cap, (int)cl.size());
        if (m > 0 && cells) std::memcpy(cells, cl.data(), sizeof(int32_t) * m);
        if (m > 0 && counts) std::memcpy(counts, ct.data(), sizeof(int32_t) * m);
        return LVI_OK;
    });
}

int32_t lvi_depth_debug_range(lvi_depth* h, int32_t* sel)
{
    if (!h || !sel) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->searched) return fail(LVI_ERR_STATE, "no range image yet");
    return guarded(h->device, [&]() -> int32_t {
        std::vector<unsigned long long> k(NBINS);
        LVI_HIP(hipMemcpyAsync(k.data(), h->range, sizeof(unsigned long long) * NBINS, hipMemcpyDeviceToHost, h->ctx.stream));
        wait(h);
        for (int b = 0; b < NBINS; b++) sel[b] = k[b] == ~0ull ? -1 : (int32_t)(unsigned)k[b];
        return LVI_OK;
    });
}

int32_t lvi_depth_debug_sphere(lvi_depth* h, lvi_pt* out, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out || (cap > 0 && !out)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if (!h->searched) return fail(LVI_ERR_STATE, "no sphere cloud yet");
    return guarded(h->device, [&]() -> int32_t {
        int n = 0;
        LVI_HIP(hipMemcpyAsync(&n, h->nsph, sizeof(int), hipMemcpyDeviceToHost, h->ctx.stream));
        wait(h);
        *n_out = n;
        const int m = std::min(cap, n);
        if (m > 0) { LVI_HIP(hipMemcpyAsync(out, h->sphere, sizeof(lvi_pt) * (size_t)m, hipMemcpyDeviceToHost, h->ctx.stream)); wait(h); }
        return LVI_OK;
    });
}

int32_t lvi_depth_debug_neighbors(lvi_depth* h, int32_t* idx, float* sqd, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *n_out = h->last_nf;
    const int m = std::min(cap, h->last_nf);
    if (m <= 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        if (idx) LVI_HIP(hipMemcpyAsync(idx, h->nbr, sizeof(int32_t) * 3 * (size_t)m, hipMemcpyDeviceToHost, h->ctx.stream));
        if (sqd) LVI_HIP(hipMemcpyAsync(sqd, h->nsqd, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, h->ctx.stream));
        wait(h);
        return LVI_OK;
    });
}

int32_t lvi_depth_set_full_search(lvi_depth* h, int32_t on)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    h->full = on != 0;
    return LVI_OK;
}

}  // extern "C"
