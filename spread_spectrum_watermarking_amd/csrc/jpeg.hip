// The JPEG attack (ssw_jpeg_rgb8): what a marked copy looks like after somebody saved it as a baseline JPEG.  include/ssw.h states
// the steps; they are libjpeg's (4:2:0, the Annex K tables scaled by its quality rule, the `islow` DCT, "fancy" upsampling)
// without the entropy coder, which is lossless.  Every quantity is an integer of at most 32 bits, so the frames equal the numpy
// restatement of tests/test_jpeg_cpu.py -- and with it PIL's save / open round trip -- exactly.  The reference has no
// counterpart: its README names JPEG compression as the attack the scheme is meant to survive and leaves measuring it to the user.
//
// Kernels (grid z: the jobs of a launch, JP_BATCH at most, their tables as kernel arguments):
//   jpeg_codec_kernel     a block owns a strip of JP_MCUS 16 x 16-pixel MCUs.  It reads the RGB bytes once (four pixels of two
//                         rows per thread and step), converts, box-filters the chroma and keeps the six 8 x 8 blocks of every MCU
//                         in LDS as 32-bit samples, rows of 9 words: with that stride the 32 lanes of an LDS access hit 32 banks
//                         whether they walk rows or columns.  Then one lane does one 8-sample line per pass: forward rows |
//                         forward columns, quantise, dequantise, inverse columns (one lane, one column: all in registers) |
//                         inverse rows, clamp, one 8-byte store into the decoded Y, Cb or Cr plane of the workspace.
//   jpeg_upsample_kernel  the triangle filter needs one chroma sample from the neighbouring blocks, hence a pass of its own: a
//                         thread reads 3 x 6 samples of Cb and Cr and 2 x 8 of Y and writes 8 x 2 RGB pixels.
// Multiplications: every product is of two values below 2^23 (samples and coefficients stay below 2^19, constants below 2^15)
// and fits 32 bits, so the 24-bit multiply (full rate) applies.  The quantiser divides by multiplying with a reciprocal
// (jpeg_tables.hpp).
#include <algorithm>

#include "jpeg_tables.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned JP_BATCH = 16;                       // jobs per launch
constexpr unsigned JP_MCUS = 16;                        // MCUs of a block's strip: 256 x 16 pixels
constexpr unsigned JP_ROW = 9;                          // words between the rows of an 8 x 8 block in LDS
constexpr unsigned JP_BLOCK = 8 * JP_ROW;               // words of a block
constexpr unsigned JP_LINES = 6 * 8;                    // 8-sample lines of an MCU and pass: 4 luma blocks, Cb, Cr
constexpr size_t JP_GROUP_BYTES = (size_t)64 << 20;     // decoded planes kept at a time (one job's, if they are more)
constexpr size_t JP_SIDE_MAX = 65535;                   // what a JPEG can hold
static_assert(JP_MCUS == 16, "the load of jpeg_codec_kernel takes 64 groups of four pixels per row");

struct JpegDesc { uint32_t frame; uint8_t q[2][64]; };  // the tables of the job's quality: luma, chroma
struct JpegBatch { JpegDesc it[JP_BATCH]; };

// FIX(x) of jfdctint.c / jidctint.c, 13 bits
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
              F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ inline int mul(int x, int k) { return __mul24(x, k); }
__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow over 8 samples; FIRST: the row pass (results scaled up by 4), else the column pass
template <bool FIRST>
__device__ inline void fdct_line(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int y1 = mul(t12 + t13, F_0_541);
    d[2] = descale(y1 + mul(t13, F_0_765), n);
    d[6] = descale(y1 - mul(t12, F_1_847), n);
    const int z5 = mul(t4 + t6 + t5 + t7, F_1_175);
    const int z1 = -mul(t4 + t7, F_0_899), z2 = -mul(t5 + t6, F_2_562);
    const int z3 = z5 - mul(t4 + t6, F_1_961), z4 = z5 - mul(t5 + t7, F_0_390);
    d[7] = descale(mul(t4, F_0_298) + z1 + z3, n);
    d[5] = descale(mul(t5, F_2_053) + z2 + z4, n);
    d[3] = descale(mul(t6, F_3_072) + z2 + z3, n);
    d[1] = descale(mul(t7, F_1_501) + z1 + z4, n);
}

// one pass of jpeg_idct_islow; FIRST: the column pass, else the row pass (which takes the remaining factor 8 out)
template <bool FIRST>
__device__ inline void idct_line(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 18;
    const int y1 = mul(d[2] + d[6], F_0_541);
    const int e2 = y1 - mul(d[6], F_1_847), e3 = y1 + mul(d[2], F_0_765);
    const int e0 = (d[0] + d[4]) * 8192, e1 = (d[0] - d[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    const int i7 = d[7], i5 = d[5], i3 = d[3], i1 = d[1];
    const int z5 = mul(i7 + i3 + i5 + i1, F_1_175);
    const int z1 = -mul(i7 + i1, F_0_899), z2 = -mul(i5 + i3, F_2_562);
    const int z3 = z5 - mul(i7 + i3, F_1_961), z4 = z5 - mul(i5 + i1, F_0_390);
    const int t0 = mul(i7, F_0_298) + z1 + z3, t1 = mul(i5, F_2_053) + z2 + z4;
    const int t2 = mul(i3, F_3_072) + z2 + z3, t3 = mul(i1, F_1_501) + z1 + z4;
    d[0] = descale(t10 + t3, n); d[7] = descale(t10 - t3, n);
    d[1] = descale(t11 + t2, n); d[6] = descale(t11 - t2, n);
    d[2] = descale(t12 + t1, n); d[5] = descale(t12 - t1, n);
    d[3] = descale(t13 + t0, n); d[4] = descale(t13 - t0, n);
}

__device__ inline uint32_t clamp_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

// the four pixels x .. x + 3 of a row as three words, the last pixel repeated beyond the frame
__device__ inline void load_px4(const uint8_t* __restrict__ row, uint32_t x, uint32_t w, uint32_t (&v)[3]) {
    if (x + 4 <= w) { __builtin_memcpy(v, row + (size_t)x * 3, 12); return; }
    uint8_t p[12];
#pragma unroll
    for (unsigned i = 0; i < 4; ++i) {
        const uint8_t* __restrict__ s = row + (size_t)min(x + i, w - 1) * 3;
        p[3 * i] = s[0]; p[3 * i + 1] = s[1]; p[3 * i + 2] = s[2];
    }
    __builtin_memcpy(v, p, 12);
}
__device__ inline int byte_of(const uint32_t* v, unsigned i) { return (int)((v[i >> 2] >> (8 * (i & 3))) & 0xFFu); }

// planes of a job in the workspace: Y [rows16][pitch] | Cb [rows16 / 2][pitch / 2] | Cr; pitch, rows16: w, h rounded up to 16
__device__ inline size_t job_planes(uint32_t pitch, uint32_t rows16) { return (size_t)pitch * rows16 * 3 / 2; }

// grid: (strips * bands of 16 rows, 1, jobs of the launch); block: 256
__global__ __launch_bounds__(256) void jpeg_codec_kernel(JpegBatch b, const uint8_t* __restrict__ frames, size_t fb, uint32_t w, uint32_t h,
                                                         uint32_t strips, uint32_t pitch, uint32_t rows16, uint8_t* __restrict__ planes) {
    __shared__ int s_blk[JP_MCUS * 6 * JP_BLOCK];
    __shared__ uint32_t s_q[128], s_m[128];                  // table entries and the reciprocals of 8 q: luma, chroma
    const unsigned t = threadIdx.x;
    const JpegDesc& d = b.it[blockIdx.z];
    if (t < 128) {
        const uint32_t q = d.q[t >> 6][t & 63];
        s_q[t] = q;
        s_m[t] = jpeg_reciprocal(8u * q);
    }
    const uint32_t band = blockIdx.x / strips, strip = blockIdx.x - band * strips;
    const uint32_t x0 = strip * (JP_MCUS * 16), y0 = band * 16;
    const uint32_t n_mcu = min(JP_MCUS, (w - x0 + 15) >> 4), lines = n_mcu * JP_LINES;
    // the band's last chroma row that the frame has: the rows below it repeat it (the DOWNSAMPLED row, not the input's)
    const uint32_t last_c = min(7u, ((h + 1) >> 1) - 1 - band * 8);
    const uint8_t* __restrict__ src = frames + (size_t)d.frame * fb;

    // ---- RGB -> Y - 128, and Cb - 128, Cr - 128 through the 2 x 2 box; a thread takes four pixels of two rows
#pragma unroll
    for (unsigned i = 0; i < JP_MCUS * 4 * 8 / 256; ++i) {
        const unsigned u = t + 256 * i, ux = u & 63, uy = u >> 6, mcu = ux >> 2;
        if (mcu >= n_mcu) continue;
        uint32_t p[2][3];
        load_px4(src + (size_t)min(y0 + 2 * uy, h - 1) * w * 3, x0 + ux * 4, w, p[0]);
        load_px4(src + (size_t)min(y0 + 2 * uy + 1, h - 1) * w * 3, x0 + ux * 4, w, p[1]);
        int* __restrict__ m = s_blk + mcu * 6 * JP_BLOCK;
        int cb[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
        for (unsigned v = 0; v < 2; ++v)
#pragma unroll
            for (unsigned k = 0; k < 4; ++k) {
                const int r = byte_of(p[v], 3 * k), g = byte_of(p[v], 3 * k + 1), bl = byte_of(p[v], 3 * k + 2);
                const unsigned lx = (ux & 3) * 4 + k, ly = 2 * uy + v;
                m[((ly >> 3) * 2 + (lx >> 3)) * JP_BLOCK + (ly & 7) * JP_ROW + (lx & 7)] = ((19595 * r + 38470 * g + 7471 * bl + 32768) >> 16) - 128;
                cb[k >> 1] += (-11059 * r - 21709 * g + 32768 * bl + (128 << 16) + 32767) >> 16;
                cr[k >> 1] += (32768 * r - 27439 * g - 5329 * bl + (128 << 16) + 32767) >> 16;
            }
        if (uy <= last_c) {
            const unsigned r_end = uy == last_c ? 7 : uy;
#pragma unroll
            for (unsigned j = 0; j < 2; ++j) {                // the rounding bias alternates 1, 2 along a row
                const unsigned cx = (ux & 3) * 2 + j;
                const int vb = ((cb[j] + 1 + (int)j) >> 2) - 128, vr = ((cr[j] + 1 + (int)j) >> 2) - 128;
                for (unsigned r = uy; r <= r_end; ++r) {
                    m[4 * JP_BLOCK + r * JP_ROW + cx] = vb;
                    m[5 * JP_BLOCK + r * JP_ROW + cx] = vr;
                }
            }
        }
    }
    __syncthreads();

    // ---- forward rows
    for (unsigned l = t; l < lines; l += 256) {
        int* __restrict__ p = s_blk + (l >> 3) * JP_BLOCK + (l & 7) * JP_ROW;
        int v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) v[k] = p[k];
        fdct_line<true>(v);
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) p[k] = v[k];
    }
    __syncthreads();

    // ---- forward columns, quantise (round half away from zero), dequantise, inverse columns
    for (unsigned l = t; l < lines; l += 256) {
        const unsigned blk = l >> 3, c = l & 7, comp = blk % 6 >= 4 ? 64 : 0;
        int* __restrict__ p = s_blk + blk * JP_BLOCK + c;
        int v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) v[k] = p[k * JP_ROW];
        fdct_line<false>(v);
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const uint32_t q = s_q[comp + k * 8 + c];
            const int level = mul((int)jpeg_divide((uint32_t)abs(v[k]) + 4u * q, s_m[comp + k * 8 + c]), (int)q);
            v[k] = v[k] < 0 ? -level : level;
        }
        idct_line<true>(v);
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) p[k * JP_ROW] = v[k];
    }
    __syncthreads();

    // ---- inverse rows, + 128, clamp: 8 bytes of one row of a plane
    uint8_t* __restrict__ plane_y = planes + (size_t)blockIdx.z * job_planes(pitch, rows16);
    uint8_t* __restrict__ plane_c = plane_y + (size_t)pitch * rows16;
    const uint32_t cpitch = pitch >> 1;
    for (unsigned l = t; l < lines; l += 256) {
        const unsigned blk = l >> 3, r = l & 7, mcu = blk / 6, yb = blk - mcu * 6;
        const int* __restrict__ p = s_blk + blk * JP_BLOCK + r * JP_ROW;
        int v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) v[k] = p[k];
        idct_line<false>(v);
        uint2 o;
        o.x = clamp_u8(v[0] + 128) | (clamp_u8(v[1] + 128) << 8) | (clamp_u8(v[2] + 128) << 16) | (clamp_u8(v[3] + 128) << 24);
        o.y = clamp_u8(v[4] + 128) | (clamp_u8(v[5] + 128) << 8) | (clamp_u8(v[6] + 128) << 16) | (clamp_u8(v[7] + 128) << 24);
        uint8_t* dst = yb < 4 ? plane_y + (size_t)(y0 + (yb >> 1) * 8 + r) * pitch + x0 + mcu * 16 + (yb & 1) * 8
                              : plane_c + (size_t)(yb - 4) * cpitch * (rows16 >> 1) + (size_t)(band * 8 + r) * cpitch + (x0 >> 1) + mcu * 8;
        *reinterpret_cast<uint2*>(dst) = o;                    // aligned: every term is a multiple of 8
    }
}

// the chroma samples cx0 - 1 .. cx0 + 4 of a row, the frame's first and last (cw - 1) repeated beyond it
__device__ inline void load_c6(const uint8_t* __restrict__ row, uint32_t cx0, uint32_t cw, int (&a)[6]) {
    if (cx0 >= 1 && cx0 + 5 <= cw) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(row + cx0);      // cx0 is a multiple of 4, the row of 8
        a[0] = row[cx0 - 1];
        a[1] = v & 0xFF; a[2] = (v >> 8) & 0xFF; a[3] = (v >> 16) & 0xFF; a[4] = v >> 24;
        a[5] = row[cx0 + 4];
        return;
    }
#pragma unroll
    for (unsigned j = 0; j < 6; ++j) a[j] = row[min(max((int)(cx0 + j) - 1, 0), (int)cw - 1)];
}

// h2v2 "fancy" upsampling of the chroma samples cx0 .. cx0 + 3 of row cy: up[v][i] is pixel (2 cx0 + i, 2 cy + v), minus 128
__device__ inline void upsample(const uint8_t* __restrict__ plane, uint32_t cpitch, uint32_t cx0, uint32_t cy, uint32_t cw, uint32_t ch,
                                int (&up)[2][8]) {
    int a[3][6];
    load_c6(plane + (size_t)(cy ? cy - 1 : 0) * cpitch, cx0, cw, a[0]);
    load_c6(plane + (size_t)cy * cpitch, cx0, cw, a[1]);
    load_c6(plane + (size_t)min(cy + 1, ch - 1) * cpitch, cx0, cw, a[2]);
#pragma unroll
    for (unsigned v = 0; v < 2; ++v) {
        int cs[6];
#pragma unroll
        for (unsigned j = 0; j < 6; ++j) cs[j] = 3 * a[1][j] + a[2 * v][j];
#pragma unroll
        for (unsigned i = 0; i < 4; ++i) {
            up[v][2 * i] = ((3 * cs[i + 1] + cs[i] + 8) >> 4) - 128;
            up[v][2 * i + 1] = ((3 * cs[i + 1] + cs[i + 2] + 7) >> 4) - 128;
        }
    }
}

// grid: (chroma columns / 256, chroma rows / 4, jobs of the launch); block: (64, 4).  out_all: [jobs of the launch][fb]
__global__ __launch_bounds__(256) void jpeg_upsample_kernel(const uint8_t* __restrict__ planes, uint32_t w, uint32_t h, uint32_t pitch,
                                                            uint32_t rows16, size_t fb, uint8_t* __restrict__ out_all) {
    const uint32_t cw = (w + 1) >> 1, ch = (h + 1) >> 1, cpitch = pitch >> 1;
    const uint32_t cx0 = (blockIdx.x * 64 + threadIdx.x) * 4, cy = blockIdx.y * 4 + threadIdx.y;
    if (cx0 >= cw || cy >= ch) return;
    const uint8_t* __restrict__ plane_y = planes + (size_t)blockIdx.z * job_planes(pitch, rows16);
    const uint8_t* __restrict__ plane_cb = plane_y + (size_t)pitch * rows16;
    const uint8_t* __restrict__ plane_cr = plane_cb + (size_t)cpitch * (rows16 >> 1);
    uint8_t* __restrict__ out = out_all + (size_t)blockIdx.z * fb;
    int cb[2][8], cr[2][8];
    upsample(plane_cb, cpitch, cx0, cy, cw, ch, cb);
    upsample(plane_cr, cpitch, cx0, cy, cw, ch, cr);
    const uint32_t x = 2 * cx0;
#pragma unroll
    for (unsigned v = 0; v < 2; ++v) {
        const uint32_t y = 2 * cy + v;
        if (y >= h) continue;
        const uint2 yy = *reinterpret_cast<const uint2*>(plane_y + (size_t)y * pitch + x);
        uint8_t px[24];
#pragma unroll
        for (unsigned i = 0; i < 8; ++i) {
            const int l = (int)(((i < 4 ? yy.x : yy.y) >> (8 * (i & 3))) & 0xFF);
            px[3 * i] = (uint8_t)clamp_u8(l + ((mul(91881, cr[v][i]) + 32768) >> 16));
            px[3 * i + 1] = (uint8_t)clamp_u8(l + ((32768 - mul(22554, cb[v][i]) - mul(46802, cr[v][i])) >> 16));
            px[3 * i + 2] = (uint8_t)clamp_u8(l + ((mul(116130, cb[v][i]) + 32768) >> 16));
        }
        uint8_t* __restrict__ dst = out + ((size_t)y * w + x) * 3;
        if (x + 8 <= w) {
            uint32_t o[6];
#pragma unroll
            for (unsigned k = 0; k < 6; ++k) o[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
            __builtin_memcpy(dst, o, 24);
        } else {
#pragma unroll
            for (unsigned i = 0; i < 8; ++i)
                if (x + i < w) { dst[3 * i] = px[3 * i]; dst[3 * i + 1] = px[3 * i + 1]; dst[3 * i + 2] = px[3 * i + 2]; }
        }
    }
}

}  // namespace ssw

extern "C" int ssw_jpeg_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_jpeg_job* jobs,
                             size_t n_jobs, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > ssw::JP_SIDE_MAX || h > ssw::JP_SIDE_MAX) return SSW_ERR_BAD_DIMS;
    if (w < 8 || h < 8) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n_jobs; ++i)
        if (jobs[i].quality < 1 || jobs[i].quality > 100 || jobs[i].frame >= n_frames) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const size_t fb = w * h * 3, cw = (w + 1) / 2, ch = (h + 1) / 2;
    const uint32_t mcus = (uint32_t)((w + 15) / 16), bands = (uint32_t)((h + 15) / 16), pitch = mcus * 16, rows16 = bands * 16;
    const uint32_t strips = (mcus + ssw::JP_MCUS - 1) / ssw::JP_MCUS;
    const size_t per_job = (size_t)pitch * rows16 * 3 / 2;
    const size_t group = std::min<size_t>({ssw::JP_BATCH, n_jobs, std::max<size_t>(1, ssw::JP_GROUP_BYTES / per_job)});
    SSW_TRY(grow(ctx->shared.jpeg, group * per_job));
    uint8_t* planes = ctx->shared.jpeg.as<uint8_t>();
    // per job: the frame in and out, and the decoded planes out and in again
    StageTimer t(ctx, SSW_STAGE_CONVERT, st, (double)n_jobs * (double)(2 * fb + 2 * (w * h + 2 * cw * ch)));
    for (size_t i0 = 0; i0 < n_jobs; i0 += group) {
        const unsigned m = (unsigned)std::min(group, n_jobs - i0);
        ssw::JpegBatch b{};
        for (unsigned i = 0; i < m; ++i) {
            b.it[i].frame = jobs[i0 + i].frame;
            ssw::jpeg_qtable(ssw::JPEG_LUMA, jobs[i0 + i].quality, b.it[i].q[0]);
            ssw::jpeg_qtable(ssw::JPEG_CHROMA, jobs[i0 + i].quality, b.it[i].q[1]);
        }
        ssw::jpeg_codec_kernel<<<dim3(strips * bands, 1, m), 256, 0, st>>>(b, dev_frames, fb, (uint32_t)w, (uint32_t)h, strips, pitch, rows16, planes);
        SSW_HIP_CHECK(hipGetLastError());
        ssw::jpeg_upsample_kernel<<<dim3((unsigned)((cw + 255) / 256), (unsigned)((ch + 3) / 4), m), dim3(64, 4), 0, st>>>(
            planes, (uint32_t)w, (uint32_t)h, pitch, rows16, fb, dev_out + i0 * fb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}
