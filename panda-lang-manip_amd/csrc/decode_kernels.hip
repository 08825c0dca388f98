// decode_kernels.hip — what Inference.predict does after the classifier
// (envs/inference/inference_cls_off_rot.py:68-107), for the context's B clouds
// on the device: per point the arg-max class, the "start" and "end" point
// sets, per set the mean of point - predicted offset un-normalised with the
// cloud's scale and centroid, and the quaternion predicted at the set's first
// point, normalised and as xyz Euler degrees.
//
// One kernel, k_cloud_decode: a workgroup of kDecodeThreads owns a cloud and
// walks its head rows once, thread t the rows t, t + T, ...  Per row the label
// (and `labels`), and where the label is in a set the f64 difference of the
// point and that set's offset into the thread's six f64 sums, the set's count
// and its lowest row (the first one met: the walk ascends).  The 6 T partial
// sums meet in an LDS tree by halving (a fixed order: include/pandasim.h), the
// counts and lowest rows -- whole numbers, any order gives the same -- by wave
// shuffles and one LDS word per wave.  Threads 0 and 1 then finish the start
// and the end set.  No atomics, nothing shared between workgroups.
//
// T = 1024: a cloud is one workgroup whatever N is, and B is tens to hundreds
// on 256 compute units, so a unit holds one workgroup at most and what hides
// the latency of the strided row reads is the number of rows in flight inside
// that workgroup -- the largest one the hardware takes.  Its 48 KiB of LDS and
// its 16 waves cost no occupancy that a second workgroup would have used.
#include <limits.h>

#include "ps_cloud_math.h"

namespace {

constexpr int kDecodeThreads = 1024;
constexpr int kDecodeWaves = kDecodeThreads / 64;
constexpr int kDecodeSums = 6;  // start x y z, end x y z

__global__ __launch_bounds__(kDecodeThreads) void k_cloud_decode(const float *head, int n, int ld, int nc,
                                                                 const float *xyz, const float *centroid,
                                                                 const float *scale, uint32_t mask0, uint32_t mask1,
                                                                 float *waypoints, float *quats, float *euler_deg,
                                                                 int32_t *counts, int32_t *labels,
                                                                 int32_t *first_idx) {
#pragma clang fp contract(off)
    __shared__ double red[kDecodeSums * kDecodeThreads];
    __shared__ int32_t s_cnt[2][kDecodeWaves], s_first[2][kDecodeWaves];
    const int t = threadIdx.x;
    const int64_t env = blockIdx.x;
    const float *rows = head + env * n * ld;
    const float *pts = xyz + env * n * 3;
    double sum[kDecodeSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt0 = 0, cnt1 = 0, first0 = INT_MAX, first1 = INT_MAX;
    for (int i = t; i < n; i += kDecodeThreads) {
        const float *row = rows + (int64_t)i * ld;
        const int label = cloud_argmax(row, nc);
        if (labels) labels[env * n + i] = label;
        const bool in0 = (mask0 >> label) & 1u, in1 = (mask1 >> label) & 1u;
        if (in0 || in1) {
            const float *p = pts + (int64_t)i * 3;
            const double x = p[0], y = p[1], z = p[2];
            if (in0) {
                sum[0] += x - (double)row[nc + 0];
                sum[1] += y - (double)row[nc + 1];
                sum[2] += z - (double)row[nc + 2];
                cnt0 += 1;
                first0 = first0 < i ? first0 : i;
            }
            if (in1) {
                sum[3] += x - (double)row[nc + 3];
                sum[4] += y - (double)row[nc + 4];
                sum[5] += z - (double)row[nc + 5];
                cnt1 += 1;
                first1 = first1 < i ? first1 : i;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kDecodeSums; c++) red[c * kDecodeThreads + t] = sum[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt0 += __shfl_down(cnt0, off);
        cnt1 += __shfl_down(cnt1, off);
        const int o0 = __shfl_down(first0, off), o1 = __shfl_down(first1, off);
        first0 = o0 < first0 ? o0 : first0;
        first1 = o1 < first1 ? o1 : first1;
    }
    if ((t & 63) == 0) {
        s_cnt[0][t >> 6] = cnt0;
        s_cnt[1][t >> 6] = cnt1;
        s_first[0][t >> 6] = first0;
        s_first[1][t >> 6] = first1;
    }
    __syncthreads();
    for (int h = kDecodeThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int c = 0; c < kDecodeSums; c++) red[c * kDecodeThreads + t] += red[c * kDecodeThreads + t + h];
        }
        __syncthreads();
    }
    if (t >= 2) return;
    // thread k finishes set k
    const int k = t;
    int count = 0, first = INT_MAX;
    for (int w = 0; w < kDecodeWaves; w++) {
        count += s_cnt[k][w];
        first = s_first[k][w] < first ? s_first[k][w] : first;
    }
    float *wp = waypoints + (env * 2 + k) * 3, *q = quats + (env * 2 + k) * 4, *e = euler_deg + (env * 2 + k) * 3;
    counts[env * 2 + k] = count;
    if (first_idx) first_idx[env * 2 + k] = count > 0 ? first : -1;
    if (count == 0) {
        wp[0] = wp[1] = wp[2] = NAN;
        q[0] = q[1] = q[2] = q[3] = NAN;
        e[0] = e[1] = e[2] = NAN;
        return;
    }
    const double sc = scale ? (double)scale[env] : 1.0;
    for (int c = 0; c < 3; c++) {
        const double mean = red[(3 * k + c) * kDecodeThreads] / (double)count;
        const double scaled = mean * sc;
        wp[c] = (float)(scaled + (centroid ? (double)centroid[env * 3 + c] : 0.0));
    }
    const float *rq = rows + (int64_t)first * ld + nc + 6 + 4 * k;
    const float qx = rq[0], qy = rq[1], qz = rq[2], qw = rq[3];
    const double n2 = ((double)qx * qx + (double)qy * qy) + ((double)qz * qz + (double)qw * qw);
    const float norm = (float)sqrt(n2);
    const float fx = qx / norm, fy = qy / norm, fz = qz / norm, fw = qw / norm;
    q[0] = fx;
    q[1] = fy;
    q[2] = fz;
    q[3] = fw;
    const double x = fx, y = fy, z = fz, w = fw, deg = 180.0 / 3.14159265358979323846;
    double sp = 2.0 * (w * y - z * x);
    sp = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);  // a NaN stays a NaN
    e[0] = (float)(atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)) * deg);
    e[1] = (float)(asin(sp) * deg);
    e[2] = (float)(atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)) * deg);
}

}  // namespace

extern "C" {

int ps_cloud_decode_waypoints(ps_ctx *c, const float *head, int n, int ld, int nc, const float *xyz,
                              const float *centroid, const float *scale, uint32_t start_mask, uint32_t end_mask,
                              float *waypoints, float *quats, float *euler_deg, int32_t *counts, int32_t *labels,
                              int32_t *first_idx, void *stream) {
    if (!c || !head || !xyz || !waypoints || !quats || !euler_deg || !counts)
        return fail(c, PS_ERR_ARG, "null argument");
    if (n < 1 || n > PS_CLOUD_MAX_DENSE_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..2^20");
    if (nc < 2 || nc > PS_CLOUD_DECODE_MAX_CLASSES) return fail(c, PS_ERR_ARG, "nc outside 2..16");
    if (ld < nc + 14 || ld > PS_CLOUD_DECODE_MAX_LD) return fail(c, PS_ERR_ARG, "ld outside nc + 14 .. 4096");
    if (start_mask == 0 || end_mask == 0 || (start_mask >> nc) != 0 || (end_mask >> nc) != 0)
        return fail(c, PS_ERR_ARG, "a class mask is empty or names a class at or above nc");
    if ((centroid == nullptr) != (scale == nullptr))
        return fail(c, PS_ERR_ARG, "centroid and scale must both be given or both be NULL");
    hipLaunchKernelGGL(k_cloud_decode, dim3((unsigned)c->num_envs), dim3(kDecodeThreads), 0, (hipStream_t)stream, head,
                       n, ld, nc, xyz, centroid, scale, start_mask, end_mask, waypoints, quats, euler_deg, counts,
                       labels, first_idx);
    return check_launch(c);
}

}  // extern "C"
