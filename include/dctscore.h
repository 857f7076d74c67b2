/*
 * dctscore.h — C ABI of libdctscore.so, the MI355X (gfx950) implementation of the
 * DCT importance-score hot path of semchan/DCT_Pruning.
 *
 * The reference has no native code: the seam this library cuts at is the Python
 * block  utils/common.py:265-274  (get_feature_hook), :283-291 (densenet hook) and
 * :299-307 (u2net input hook):
 *
 *     c = [dct.dct_2d(output[i,j,:,:], norm='ortho') for i in range(a) for j in range(b)]
 *     c = cnt_score(c)            # per map: sum(coeff * coeff)      (utils/common.py:249-255)
 *     c = c.view(a, -1)           # [N, C] per-map energies
 *
 * i.e. "feature-map tensor on the device -> one fp32 energy per (sample, channel)".
 * Everything after that (sum over the batch, running mean, np.save) stays on the host in
 * Python exactly as the reference does it (utils/common.py:271-277).
 *
 * Conventions
 *   - All pointers are DEVICE pointers (hipMalloc'd / torch CUDA tensors). The caller owns
 *     every buffer; the library allocates no device memory. Its only state, all on the HOST:
 *       (1) a 16-entry memo of which byte range of which caller workspace holds the direct
 *           kernel's cosine-basis tables (per workspace pointer, stream and tile shape; see
 *           dcts_workspace_invalidate - a caller that writes into a workspace or frees it
 *           must say so);
 *       (2) values read ONCE per process: the device's CU count and per-kernel occupancy, and
 *           the environment variable DCTS_SPLIT_CHUNK_MB (size of the two-launch split path's
 *           intermediate buffer, default 256).
 *   - Strides are in ELEMENTS (floats), as torch.Tensor.stride() reports them.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). Every entry
 *     point only ENQUEUES work on that stream; there is no implicit synchronisation.
 *   - Return value: 0 = ok; negative = DCTS_E_* (bad argument / unsupported shape);
 *     positive = a hipError_t raised by the launch. Nothing throws, aborts or prints.
 *   - Re-entrant and thread-safe; safe to call with the Python GIL released.
 */
#ifndef DCTSCORE_H_
#define DCTSCORE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: workspace contract (the library may leave basis tables in a workspace between calls; 16-byte
 *    alignment; dcts_workspace_invalidate[_range]), multi / mixed / weighted entry points.
 * 3: dcts_rank_f32 (the HRank criterion) and DCTS_RANK_MAX_EDGE. The band entry points (dcts_band_energy_f32,
 *    dcts_band_workspace_bytes, dcts_has_band_kernel, DCTS_BAND_MAX) were added to 3 WITHOUT a bump: they are purely
 *    additive, and a library that lacks them fails at symbol lookup. The same holds for the fp16 / bf16 entry points
 *    (dcts_energy_typed, dcts_typed_workspace_bytes, dcts_has_half_kernel, DCTS_DTYPE_*) and for the channels-last ones
 *    (dcts_energy_nhwc, dcts_nhwc_workspace_bytes, dcts_has_nhwc_kernel), and for the spectral-entropy ones
 *    (dcts_spectral_entropy_f32, dcts_entropy_workspace_bytes, dcts_has_entropy_kernel), and for the geometric-median
 *    criterion's entry point (dcts_gm_distance_f32) and its normalised metrics (dcts_gm_distance_metric_f32,
 *    dcts_gm_workspace_bytes, DCTS_GM_*) and its pair matrix (dcts_gm_pairs_f32, dcts_gm_pairs_workspace_bytes,
 *    dcts_gm_pairs_slices), and for the low-pass signature (dcts_dct2d_lowpass_f32, dcts_dct2d_lowpass_workspace_bytes,
 *    DCTS_LOWPASS_DROP_DC). */
#define DCTS_ABI_VERSION 3

enum {
  DCTS_OK = 0,
  DCTS_E_NULL = -1,        /* a required pointer is NULL                                */
  DCTS_E_SHAPE = -2,       /* N, C, H or W <= 0, or H/W beyond DCTS_MAX_EDGE            */
  DCTS_E_CHANNELS = -3,    /* [c_begin, c_begin + c_count) not inside [0, C_total)      */
  DCTS_E_STRIDE = -4,      /* innermost stride != 1 or row stride < W (rows must be dense) */
  DCTS_E_WORKSPACE = -5,   /* workspace smaller than dcts_workspace_bytes() reports     */
  DCTS_E_UNSUPPORTED = -6, /* combination not implemented (see dcts_strerror)           */
  DCTS_E_ALIGN = -7        /* pointer not aligned to its element size (fp32: 4 bytes)   */
};

/* Largest tile edge (after the optional odd front pad) any kernel accepts. */
#define DCTS_MAX_EDGE 512

/* Kernel family selector for dcts_energy_f32_ex (testing / benchmarking). */
enum {
  DCTS_ALGO_AUTO = 0,     /* pick the fastest kernel that supports the shape                     */
  DCTS_ALGO_DIRECT = 1,   /* cosine-basis-in-LDS separable kernel, any (H, W) <= DCTS_MAX_EDGE   */
  DCTS_ALGO_CODELET = 2,  /* register-resident factorised DCT codelets (selected tile sizes)     */
  DCTS_ALGO_SPLIT = 3,    /* two-launch split codelet passes for edges 4*M / 8*M (68 ... 512)    */
  DCTS_ALGO_PREFETCH = 4, /* codelet kernel with direct-to-LDS prefetch of the next maps (dense,
                             even-edge square tiles; measured equal to ALGO_CODELET, opt-in)     */
  DCTS_ALGO_FUSED = 5,    /* single-launch split kernel, intermediate tile parked in VGPRs
                             (edges 72 ... 256 incl. 96 and 192; 288 and 320 with two roles per wave) */
  DCTS_ALGO_PIPE = 6,     /* the fused kernel software-pipelined: pass 2 of one map interleaved
                             with pass 1 of the next                                             */
  DCTS_ALGO_LANE = 7,     /* one lane per map, both passes in registers (7x7, 9x9)              */
  DCTS_ALGO_TILE2D = 8,   /* 2-D radix split: butterflies over both axes in registers, then 4^L independent
                             M x M leaf blocks - 224 (tile2d.hip); 72, 80, 96, 112, 128, 144, 160 with several maps
                             per round (tile2g.hip)                                              */
  DCTS_ALGO_RECT = 9      /* the 1-D codelets picked per axis at run time: any (H, W) with both edges (after the
                             odd pad) <= 64 - non-square maps, odd / prime edges, rows with strideH > W
                             (rect.hip); what AUTO takes for such shapes                           */
};

/* ABI version of the loaded library (== DCTS_ABI_VERSION it was built with). */
int dcts_version(void);

/* Human-readable text for a return code of this library (never NULL). */
const char* dcts_strerror(int code);

/*
 * Scratch bytes dcts_energy_f32 needs for a call with these sizes (may be 0). The caller
 * allocates it once and may reuse it across calls on the same stream.
 */
size_t dcts_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W);

/*
 * Per-map DCT energy.  Replaces utils/common.py:267 + :249-255 (and :285 / :301 through
 * torch2dct, :230-239, when pad_front_if_odd != 0).
 *
 *   x            fp32 feature maps, logical shape [N, C_total, H, W]; element (n,c,h,w) is at
 *                x[n*strideN + c*strideC + h*strideH + w*strideW]; strideW must be 1, strideH >= W.
 *                Any (H, W) <= DCTS_MAX_EDGE is accepted; which kernel runs depends on the shape: square
 *                dense maps of the tabulated edges have their own kernels, non-square maps and maps with
 *                strideH > W with both edges <= 64 the run-time codelet pair (DCTS_ALGO_RECT: any
 *                edge 1 ... 64), everything else the cosine-matrix kernel (DCTS_ALGO_DIRECT).
 *   c_begin,
 *   c_count      channel slice to score (densenet hook: c_begin = C_total-12, c_count = 12).
 *   pad_front_if_odd
 *                0: transform the H x W map as is (torch_dct path).
 *                1: cv2 path of torch2dct — if H is odd, one zero row is put in front of the
 *                   rows AND one zero column in front of the columns before the transform
 *                   (np.pad(t,(1,0)) pads every axis; the test is on H only).
 *   out_nc       [N, c_count] fp32, row-major:
 *                out_nc[n*c_count + j] = sum_{u,v} DCT2_ortho(x[n, c_begin+j])[u,v]^2
 *   workspace    >= dcts_workspace_bytes(N, c_count, H, W) bytes of device memory, 16-byte aligned,
 *                or NULL when that is 0. (The size of the two-launch split path's intermediate
 *                buffer, and with it dcts_workspace_bytes for edges 72..320, follows the environment
 *                variable DCTS_SPLIT_CHUNK_MB, read once per process; default 256.)
 */
int dcts_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                    int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                    int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                    float* out_nc, void* workspace, size_t workspace_bytes, void* stream);

/* Same, with an explicit kernel family (DCTS_ALGO_*). DCTS_E_UNSUPPORTED if that family
 * has no kernel for the shape. */
int dcts_energy_f32_ex(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                       int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                       int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                       float* out_nc, void* workspace, size_t workspace_bytes, void* stream,
                       int32_t algo);

/* The library keeps immutable basis tables at the head of a workspace between calls (built once per
 * workspace, stream and tile shape; remembered on the host, nothing is read back). A caller that writes into a
 * workspace itself, or frees it and allocates another at the same address, says so here first. */
void dcts_workspace_invalidate(void* workspace);
/* The same for callers that wrote into (or are about to free) bytes [workspace, workspace + bytes): also
 * forgets tables cached under other pointers that overlap the range. */
void dcts_workspace_invalidate_range(void* workspace, size_t bytes);

/* 1 if DCTS_ALGO_CODELET has a kernel for an (H, W) tile (sizes AFTER the odd pad). */
int dcts_has_codelet(int64_t H, int64_t W);

/*
 * Full coefficient output (parity/debug and the coefficient-domain API the reference's
 * commented-out variants hint at, utils/common.py:268-269). Same addressing as above;
 *   out_coeff    [N, c_count, H', W'] fp32 dense, H' = H + (pad && H odd), W' likewise;
 *                out_coeff[n,j] = dct_2d(x[n, c_begin+j], norm='ortho').
 *   workspace    as for dcts_energy_f32 (same size query). With DCTS_ALGO_FUSED / DCTS_ALGO_TILE2D
 *                (dcts_dct2d_f32_ex) the large-tile energy kernels themselves produce the coefficients
 *                (leaf outputs into the workspace, then the DCT-IV add/sub layers the energy path folds
 *                into its reduction): the workspace must be 16-byte aligned and hold at least one
 *                H' x W' fp32 tile; more tiles mean fewer launches.
 */
int dcts_dct2d_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                   int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                   int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                   float* out_coeff, void* workspace, size_t workspace_bytes, void* stream);

/* Same, with an explicit kernel family (DCTS_ALGO_*). */
int dcts_dct2d_f32_ex(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                      int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                      int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                      float* out_coeff, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t algo);

/*
 * Score variant in the coefficient domain (the reference only hints at variants, utils/common.py:268-269;
 * SURVEY.md §8 f4): out_nc[n, j] = sum_{u,v} weights[u, v] * dct_2d(x[n, c_begin+j], norm='ortho')[u, v]^2,
 * `weights` a dense [H', W'] fp32 device array (all ones reproduces dcts_energy_f32 up to rounding).
 * Coefficients come from the same kernels as dcts_dct2d_f32_ex (the large-tile kernels' own coefficient path
 * for dense 72..320 tiles). Workspace: dcts_weighted_workspace_bytes(), 16-byte aligned.
 */
size_t dcts_weighted_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W);
int dcts_weighted_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                             int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                             int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                             const float* weights, float* out_nc, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * K weighted energies per map in ONE pass over the data (band.hip). With c = dct_2d(x[n, c_begin+j], norm='ortho')
 * (H' x W' after the optional odd front pad) and `weights` a dense [K, H', W'] fp32 device array:
 *
 *     out_nck[(n*c_count + j)*K + b] = sum_{u,v} weights[b, u, v] * c[u, v]^2        [N, c_count, K] fp32, dense
 *
 * One-hot weights make that the energy of K frequency bands (dct_pruning_amd/bands.py builds the partitions); all
 * ones with K = 1 is dcts_energy_f32 up to rounding, K = 1 in general is dcts_weighted_energy_f32's score.
 *   K          1 ... DCTS_BAND_MAX, else DCTS_E_SHAPE. Weights are arbitrary floats.
 *   x, strides, c_begin, c_count, pad_front_if_odd    as for dcts_energy_f32; any (H, W) <= DCTS_MAX_EDGE.
 *   algo       DCTS_ALGO_AUTO     the fused kernel where it exists (square tiles with a codelet,
 *                                 dcts_has_band_kernel(H', W') == 1, rows dense: strideH == W), else the fallback;
 *              DCTS_ALGO_CODELET  the fused kernel only (DCTS_E_UNSUPPORTED otherwise);
 *              DCTS_ALGO_DIRECT   the fallback only: coefficients of a chunk of maps through the coefficient path
 *                                 (dcts_dct2d_f32_ex's kernels) into the workspace, then one reduction that reads
 *                                 each coefficient once for all K bands.
 *   workspace  >= dcts_band_workspace_bytes(N, c_count, H, W, K) bytes, 16-byte aligned, never NULL. The fused kernel
 *              keeps the re-laid weight table (at most 128 KiB) at its head; the fallback chunks by what it is given.
 * A map's K values depend on nothing but that map and the weights (not on N, the channel slice, K's rounding, the
 * other maps or the launch count): bit-reproducible, no atomics. An all-zero map gives +0.0 in every band (finite
 * weights); a NaN / Inf map affects only its own K outputs. Only enqueues on `stream`.
 */
#define DCTS_BAND_MAX 8
size_t dcts_band_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W, int32_t K);
/* 1 if the fused band kernel takes an (H, W) tile (sizes AFTER the odd pad). */
int dcts_has_band_kernel(int64_t H, int64_t W);
int dcts_band_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                         int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                         int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                         const float* weights, int32_t K, float* out_nck, void* workspace, size_t workspace_bytes,
                         void* stream, int32_t algo);

/*
 * The spectral entropy of every map (entropy.hip): how widely a map's energy spreads over its DCT coefficients. With
 * c = dct_2d(x[n, c_begin+j], norm='ortho') (H' x W' after the optional odd front pad), E = sum c^2 and p = c^2 / E:
 *
 *     out_nc[n*c_count + j] = -sum_{p[u,v] > 0} p[u, v] * ln p[u, v]                  [N, c_count] fp32, dense
 *
 * Natural logarithm; the value lies in [+0.0, ln(H' * W')] (both ends enforced): near 0 for a flat or blob-like map,
 * near ln(H' * W') for a textured one. It does not change when the map is scaled. An all-zero map gives exactly +0.0.
 * All arithmetic is fp32 with the accurate logf, in one pass: e = sum w^2, s = sum w^2 ln w^2 (zero squares add
 * nothing), H = ln e - s / e, on whatever common scale w the kernel's coefficients have.
 *   x, strides, c_begin, c_count, pad_front_if_odd    as for dcts_energy_f32; any (H, W) <= DCTS_MAX_EDGE.
 *   algo       DCTS_ALGO_AUTO     the fused kernel where it exists (square tiles with a codelet,
 *                                 dcts_has_entropy_kernel(H', W') == 1, rows dense: strideH == W), else the fallback;
 *              DCTS_ALGO_CODELET  the fused kernel only (DCTS_E_UNSUPPORTED otherwise);
 *              DCTS_ALGO_DIRECT   the fallback only: coefficients of a chunk of maps through the coefficient path
 *                                 (dcts_dct2d_f32_ex's kernels) into the workspace, then one reduction that reads
 *                                 each coefficient once.
 *   workspace  >= dcts_entropy_workspace_bytes(N, c_count, H, W) bytes, 16-byte aligned; that is 0 where the fused kernel
 *              takes the shape (with and without the odd pad), and NULL is then fine. A call of such a shape that the
 *              fused kernel does not take (rows with a pitch, DCTS_ALGO_DIRECT) goes through the fallback: size its
 *              workspace as for (H, W + 1), which is never fused and never needs less. The fallback chunks by what it is
 *              given; DCTS_E_WORKSPACE if that is less than the coefficient path's own need plus two tiles.
 * A map's value depends on that map alone (not on N, the channel slice, its position in a wave, the launch count or the
 * chunking): bit-reproducible, no atomics. A NaN / Inf map affects only its own output. Only enqueues on `stream`; no
 * new host state.
 */
size_t dcts_entropy_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W);
/* 1 if the fused entropy kernel takes an (H, W) tile (sizes AFTER the odd pad). */
int dcts_has_entropy_kernel(int64_t H, int64_t W);
int dcts_spectral_entropy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                              int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                              int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                              float* out_nc, void* workspace, size_t workspace_bytes, void* stream, int32_t algo);

/*
 * The geometric-median criterion on feature maps (gm.hip): FPGM prunes the filter whose weights lie closest to the geometric
 * median of its layer, the element whose summed distance to all the others is smallest. Applied to the maps a layer produces:
 *
 *     out_nc[n*c_count + j] = sum_{k = r_begin}^{r_begin+r_count-1} || x[n, c_begin+j] - x[n, k] ||_2     [N, c_count] fp32, dense
 *
 * the Euclidean norm over the H * W elements of a map. High = far from the other maps of the reference set = keep, so "keep
 * the highest scores" holds as for every other criterion. The only entry point whose value looks at a second channel.
 *   c_begin, c_count    the scored maps;  r_begin, r_count   the reference set they are compared with. Both ranges lie inside
 *              [0, C_total) (DCTS_E_CHANNELS otherwise). They are separate so that a caller who cuts a layer into channel ranges
 *              can still compare every piece with the whole layer.
 *   x, strides   addressed as for dcts_energy_f32, but the maps must be dense: strideW == 1 and strideH == W (strideW != 1 or
 *              strideH < W: DCTS_E_STRIDE; strideH > W: DCTS_E_UNSUPPORTED, the copy stays with the caller). strideN and
 *              strideC may be anything; x any 4-byte-aligned address (DCTS_E_ALIGN otherwise). Any 1 <= H, W <= DCTS_MAX_EDGE.
 *              All offsets are computed in 64 bits. One workgroup serves a sample and 64 scored channels; a call that needs
 *              more than 2^31 - 1 of them returns DCTS_E_SHAPE.
 *   There is no pad_front_if_odd: a zero row and a zero column in front of BOTH maps add zeros to the sum of squared
 *              differences, so the odd front pad is a no-op by construction.
 * Arithmetic, all fp32 VALU: the DIFFERENCE form d^2 = sum_p (a_p - b_p)^2, one fused multiply-add chain per pair with p
 * ascending, d = sqrtf(d^2), then a fixed-order sum over k. Never the Gram form |a|^2 + |b|^2 - 2 a.b, which cancels for the
 * near-duplicate pairs the criterion exists to find. Hence: the k == c term is exactly 0; two identical maps are at distance
 * exactly +0.0; an all-zero sample gives +0.0 everywhere; d(a, b) has the same bits whichever map is scored and whichever is
 * the reference.
 * out[n, j] depends on the scored map and on the reference set of sample n only: not on N, not on c_begin / c_count (pieces
 * of a channel range concatenate to the unsplit result bit for bit), not on the map's position in a tile or the launch
 * count. No atomics. A NaN / Inf map poisons the outputs of its own sample only (it is a term of each of them).
 * No workspace, no host state; only enqueues on `stream`; the arguments are checked before any launch.
 */
int dcts_gm_distance_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                         int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                         int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count,
                         float* out_nc, void* stream);

/*
 * dcts_gm_distance_f32 under another metric: the same sum over UNIT maps, so that the pattern of a map is compared and not its
 * gain (the plain distance obeys ||a - b|| >= | ||a|| - ||b|| |: a map with a large norm is far from everything).
 *
 *     out_nc[n*c_count + j] = sum_{k = r_begin}^{r_begin+r_count-1} || u[n, c_begin+j] - u[n, k] ||_2,   every term in [0, 2]
 *
 *   DCTS_GM_L2           u = x: dcts_gm_distance_f32 itself, bit for bit; no workspace (NULL / 0 are fine).
 *   DCTS_GM_COSINE       u = x / ||x||_2                        d^2 = 2 - 2 cos(a, b)
 *   DCTS_GM_CORRELATION  u = (x - mu) / ||x - mu||_2, mu the mean of the map    d^2 = 2 - 2 rho (Pearson)
 *   Flat maps: a map with nothing to normalise has u = 0, every element exactly +0.0. For the cosine that is a map with
 *              sum x^2 == 0; for the correlation a map whose maximum equals its minimum (an exact comparison, no threshold on
 *              the centred sum). A flat map is at distance 1 (to rounding) from every map that is not flat and at exactly 0 from
 *              every other flat map: dead channels score low, next to the duplicates. High = far = keep, as ever.
 *   metric     any other value: DCTS_E_UNSUPPORTED.
 *   workspace  device memory, 16-byte aligned, at least dcts_gm_workspace_bytes(metric, N, c_count, r_count) bytes (0 for
 *              DCTS_GM_L2): one (mu, 1 / norm) pair per scored and per reference map, written by a launch of their own before the
 *              distances. The call overwrites it; a workspace shared with the other entry points is handled as theirs
 *              (dcts_workspace_invalidate[_range] for memory that is freed or written by the caller).
 *   Checks, in this order: everything dcts_gm_distance_f32 checks, in its order; the metric; the workspace (NULL or too small:
 *              DCTS_E_WORKSPACE; not 16-byte aligned: DCTS_E_ALIGN). A call that needs more than
 *              2^31 - 1 workgroups in either launch (4 maps or 64 scored channels of a sample each) returns DCTS_E_SHAPE.
 * Arithmetic, all fp32: mu = sum / (H*W); the norm from a SECOND pass over the map, sum (x - mu)^2, never sum x^2 - H*W*mu^2;
 * every sum in an order that depends on the element's index and on H*W alone. u = (x - mu) * (1 / norm), rounded once. Then the
 * difference form of dcts_gm_distance_f32, with what it makes exact: the k == c term, identical maps, d(a, b) against d(b, a).
 * New: a map and a power-of-two multiple of it are at distance exactly +0.0 (sum (2^k x)^2 = 4^k sum x^2, and the correctly
 * rounded square root and division commute with that scaling), for every k that makes nothing denormal or overflow.
 * Everything dcts_gm_distance_f32 says about independence holds: out[n, j] does not depend on N, c_begin / c_count, the launch
 * or the alignment of x. A NaN map poisons its own sample only.
 * Limit: the centring is done in fp32. A map that is nearly constant without being flat (spread within a few ulp of its
 * mean) has a unit map that is mostly rounding; the criterion is not meaningful there, and the tests hold no such map.
 * Only enqueues on `stream`: no allocation, no atomics; the arguments are checked before any launch.
 */
#define DCTS_GM_L2 0
#define DCTS_GM_COSINE 1
#define DCTS_GM_CORRELATION 2
size_t dcts_gm_workspace_bytes(int32_t metric, int64_t N, int32_t c_count, int32_t r_count);
int dcts_gm_distance_metric_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                                int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                                int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count,
                                float* out_nc, void* stream, int32_t metric, void* workspace, size_t workspace_bytes);

/*
 * The terms of dcts_gm_distance_metric_f32 instead of their sum over the reference set, summed over the SAMPLES (gm_pairs.hip):
 *
 *     out_cr[j*r_count + k] = sum_{n = 0}^{N-1} d(x[n, c_begin+j], x[n, r_begin+k])        [c_count, r_count] fp32, dense
 *
 * d the distance of dcts_gm_distance_metric_f32 under `metric` (DCTS_GM_L2: the maps as they are; DCTS_GM_COSINE,
 * DCTS_GM_CORRELATION: their unit maps, flat maps as described there). A row sum cannot tell two duplicates that are far from
 * everything else from two distinct far maps; the matrix can, and every selection rule on it (nearest neighbour, farthest
 * point, clustering) is host arithmetic. It is a SUM over the samples, not a mean: the caller owns the count. One matrix per
 * sample is not offered: [N, C, C] floats are 4 GiB for 2048 channels at batch 256. The call overwrites out_cr.
 *   x, strides, the two channel ranges, metric     as for dcts_gm_distance_metric_f32.
 *   Slices     the samples are cut into S = dcts_gm_pairs_slices(N, r_count) contiguous runs of ceil(N / S) samples (the last
 *              one shorter, none empty), each summed with n ascending by a workgroup of its own so that a narrow layer still
 *              fills the GPU; the S partial matrices are then added with s ascending. 1 <= S <= N; S depends on N and r_count
 *              alone (0 for N <= 0 or r_count <= 0): not on the scored range, the alignment of x or the device.
 *   workspace  device memory, 16-byte aligned, at least dcts_gm_pairs_workspace_bytes(metric, N, c_count, r_count) bytes: the
 *              (mu, 1 / norm) pairs of a metric, laid out as dcts_gm_distance_metric_f32 has them, then the S partial matrices
 *              where S > 1. 0 for DCTS_GM_L2 with S == 1, where NULL / 0 are fine and the one launch stores to out_cr itself.
 *              The query returns 0 for a metric it does not know. Handled as the other entry points' workspace.
 *   Checks, in this order: everything dcts_gm_distance_f32 checks, in its order (out_cr in the place of out_nc); the metric
 *              (DCTS_E_UNSUPPORTED); the workspace (NULL or too small: DCTS_E_WORKSPACE; not 16-byte aligned: DCTS_E_ALIGN);
 *              then the grids: a launch of more than 2^31 - 1 workgroups returns DCTS_E_SHAPE before anything is enqueued.
 * Arithmetic: every pair exactly as in dcts_gm_distance_f32 / dcts_gm_distance_metric_f32 (the difference form, two fused
 * multiply-add chains with p ascending, sqrtf), then fp32 additions in the order above. Hence, bit for bit: the entry of a
 * channel with itself is +0.0; two identical maps are at +0.0 (under a metric, a map and a power-of-two multiple of it);
 * an all-zero tensor gives +0.0 everywhere; with the scored range equal to the reference range out[j, k] has the bits of
 * out[k, j]; a row of a call on a sub-range of the scored channels has the bits it has in the call on the whole range with the
 * same reference range; the bits do not depend on the alignment of x. A NaN / Inf map reaches its own row and column only.
 * Only enqueues on `stream`: two to four launches at most, no allocation, no atomics; the arguments are checked first.
 */
size_t dcts_gm_pairs_workspace_bytes(int32_t metric, int64_t N, int32_t c_count, int32_t r_count);
int32_t dcts_gm_pairs_slices(int64_t N, int32_t r_count);
int dcts_gm_pairs_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                      int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                      int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count,
                      float* out_cr, void* stream, int32_t metric, void* workspace, size_t workspace_bytes);

/*
 * The low-pass DCT signature of every map (lowpass.hip): the corner of the lowest frequencies of dcts_dct2d_f32's output,
 *
 *     out[((n*c_count + j)*Kh + u)*Kw + v] = dct_2d(x[n, c_begin+j], norm='ortho')[u][v],   u < Kh = min(K, H), v < Kw = min(K, W)
 *
 * [N, c_count, Kh, Kw] fp32, dense, and nothing else: a map is read once and Kh*Kw floats are written. The distance between
 * two signatures, || P_K DCT(a) - P_K DCT(b) ||_2, is the band-limited form of the distance dcts_gm_distance_f32 takes (which
 * the orthonormal transform leaves unchanged when every coefficient is kept): the gm entry points take `out` as their tensor.
 *   x, strides, c_begin, c_count    as for dcts_energy_f32 (strideW == 1, strideH >= W). There is no odd front pad.
 *   K          >= 1 (DCTS_E_SHAPE otherwise). An edge shorter than K keeps all its coefficients: Kh = H, Kw = W there.
 *   flags      0, or DCTS_LOWPASS_DROP_DC; any other bit: DCTS_E_UNSUPPORTED. With DCTS_LOWPASS_DROP_DC, out[.., 0, 0] is
 *              written as +0.0 (the signature of the centred map), and a FLAT map - every element equal to the first, all-zero
 *              maps included - gets an all-+0.0 signature. The test is made on the map itself and is exact: the AC coefficients of
 *              a constant map are exactly 0 for power-of-two edges only, and the round-off the other edges leave there would,
 *              normalised, be a unit vector of noise. A map that holds a NaN is not flat. Every other element has the bits it
 *              has without the flag.
 *   workspace  device memory, 16-byte aligned, at least dcts_dct2d_lowpass_workspace_bytes(N, c_count, H, W, K) bytes. That is 0
 *              for dense square maps of an edge dcts_has_codelet names, which one fused launch serves (NULL is fine). Every
 *              other shape up to DCTS_MAX_EDGE takes the coefficient path of dcts_dct2d_f32 chunk by chunk into the workspace
 *              and a gather of the corners; so does a codelet shape whose rows have a pitch: size its workspace as for
 *              (H, W + 1), which is never fused and never needs less. The call overwrites the workspace; one shared with the
 *              other entry points is handled as theirs (dcts_workspace_invalidate[_range]).
 *   Checks, in this order: everything dcts_energy_f32 checks, in its order; K; flags; then, on the fallback only, the workspace
 *              (NULL or too small: DCTS_E_WORKSPACE; not 16-byte aligned: DCTS_E_ALIGN). All before any launch.
 * A map's signature depends on that map alone: the same bits for any N, channel slice, position in a wave, chunk or launch
 * count; no atomics; a NaN map touches only its own signature. On the fallback the signature is the corner of dcts_dct2d_f32's
 * output bit for bit; the fused kernel's agrees with it to the kernels' rounding (2e-6 of the largest coefficient).
 * Only enqueues on `stream`; no host state beyond the workspace memo of the other entry points.
 */
#define DCTS_LOWPASS_DROP_DC 1
size_t dcts_dct2d_lowpass_workspace_bytes(int64_t N, int32_t c_count, int64_t H, int64_t W, int32_t K);
int dcts_dct2d_lowpass_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                           int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                           int32_t c_begin, int32_t c_count, int32_t K, int32_t flags,
                           float* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * dcts_energy_f32 for feature maps of another element type: what a forward pass under autocast hands to a hook.
 *
 *   dtype      DCTS_DTYPE_F32 forwards to dcts_energy_f32 (x is then a const float*); DCTS_DTYPE_F16 (IEEE binary16) and
 *              DCTS_DTYPE_BF16 (bfloat16) are scored as described below; anything else returns DCTS_E_UNSUPPORTED.
 *   x, strides, c_begin, c_count, pad_front_if_odd, out_nc    as for dcts_energy_f32. Strides are in ELEMENTS of `dtype`;
 *              x must be aligned to the element size (DCTS_E_ALIGN otherwise). out_nc is always fp32.
 * Every element is converted to fp32 exactly (both conversions are exact, fp16 subnormals included) and all arithmetic is
 * fp32: the result is that of dcts_energy_f32 on the upcast tensor up to the kernels' rounding.
 *   - Dense square maps (strideH == W, no odd pad taken) of the edges dcts_has_half_kernel names - 2, 4, 7, 8, 14, 16, 28,
 *     32, 56: every hook point of the six classification nets - have a kernel of their own (half.hip) that reads the 2-byte
 *     elements straight from memory: the codelet kernel's schedule with another load. No workspace (NULL is fine).
 *   - Every other shape up to DCTS_MAX_EDGE is staged: a chunk of maps of the scored slice is upcast into the workspace
 *     (dense, 16-byte aligned) and scored by dcts_energy_f32's own kernels; whole samples per chunk where the workspace
 *     holds one, runs of channels of one sample otherwise. Bit for bit what dcts_energy_f32 gives for a dense 16-byte
 *     aligned fp32 copy of the slice.
 *   workspace  >= dcts_typed_workspace_bytes(dtype, N, c_count, H, W) bytes, 16-byte aligned; that is 0 where the native
 *              kernel takes the shape. A call of such a shape that the native kernel does not take (rows with a pitch,
 *              7 x 7 with the odd pad) is staged too: size its workspace as for (H, W + 1), which is never native and
 *              never needs less. The staged route chunks by what it is given (at most 64 MiB of upcast maps per chunk);
 *              DCTS_E_WORKSPACE if that is less than the fp32 path's own need plus one upcast map.
 * A map's value depends on that map alone (not on N, the channel slice, the other maps or the launch count): no atomics,
 * +0.0 for an all-zero map, a NaN map touches only its own output. Only enqueues on `stream`; no new host state.
 */
enum { DCTS_DTYPE_F32 = 0, DCTS_DTYPE_F16 = 1, DCTS_DTYPE_BF16 = 2 };
int dcts_energy_typed(const void* x, int32_t dtype, int64_t N, int64_t C_total, int64_t H, int64_t W,
                      int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                      int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                      float* out_nc, void* workspace, size_t workspace_bytes, void* stream);
size_t dcts_typed_workspace_bytes(int32_t dtype, int64_t N, int64_t C_count, int64_t H, int64_t W);
/* 1 if the native fp16 / bf16 kernel takes a dense (H, W) map (no odd pad). */
int dcts_has_half_kernel(int64_t H, int64_t W);

/*
 * Per-map DCT energy of CHANNELS-LAST feature maps (torch.channels_last; what NHWC convolutions hand to a hook), read
 * where they lie instead of through a transposing copy (nhwc.hip).
 *
 *   x          logical shape [N, C_total, H, W] of `dtype` elements (DCTS_DTYPE_F32, _F16 or _BF16; anything else returns
 *              DCTS_E_UNSUPPORTED); element (n, c, h, w) is at x[n*strideN + h*strideH + w*strideW + c]: the channel
 *              stride is 1. strideW >= C_total and strideH >= W*strideW (DCTS_E_STRIDE otherwise). strideW may exceed the
 *              channel count and x may sit at any element offset, so a channel-sliced view of a channels-last tensor is
 *              fine. Strides are in ELEMENTS of `dtype`; x is aligned to the element size (DCTS_E_ALIGN otherwise).
 *   c_begin, c_count    channel slice to score, inside [0, C_total).
 *   out_nc     [N, c_count] fp32 as for dcts_energy_f32. There is no odd front pad.
 *   workspace  unused: dcts_nhwc_workspace_bytes() is 0 for every shape the entry point takes. NULL is fine.
 * Shapes: dense square maps of the edges dcts_has_nhwc_kernel names - 2, 4, 7, 8 (one lane holds one map: the 64 lanes
 * of a wave are 64 consecutive channels) and 14, 16, 28, 32 (a block of 32 / 32 / 16 / 8 channels of one sample goes
 * through LDS, then the codelet kernels' schedule) and 56 (4 channels, strips of 8 rows through LDS, one wave per
 * map). Every other shape returns DCTS_E_UNSUPPORTED: the
 * copy into the NCHW layout stays with the caller.
 * Every element is converted to fp32 exactly and all arithmetic is fp32. A map's value depends on that map alone (not on
 * N, C_total, the channel slice, its position in a wave or block, or the launch count): no atomics, +0.0 for an
 * all-zero map, a NaN map touches only its own output. The value is that of dcts_energy_f32 / dcts_energy_typed on the
 * NCHW copy up to the kernels' rounding (same codelets; the summation order differs at 2, 4, 7, 8).
 * Only enqueues on `stream`; no host state.
 */
int dcts_has_nhwc_kernel(int64_t H, int64_t W);
size_t dcts_nhwc_workspace_bytes(int32_t dtype, int64_t N, int64_t C_count, int64_t H, int64_t W);
int dcts_energy_nhwc(const void* x, int32_t dtype, int64_t N, int64_t C_total, int64_t H, int64_t W,
                     int64_t strideN, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                     float* out_nc, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Fused batch reduction for benchmarking and for the single-sweep harness:
 *   out_c[j] = sum_n energy[n, j]   (fp32; summation order: 16 interleaved slices, slice s adds
 *   n = s, s+16, s+32, ... in ascending order, then the 16 partial sums are added in slice order.
 *   Fixed, launch-independent and bit-reproducible, but not torch's c.view(a,-1).sum(0) order: the
 *   reference-exact path is dcts_energy_f32 + host-side sum(0), utils/common.py:271-274).
 */
int dcts_batch_sum_f32(const float* energy_nc, int64_t N, int64_t C_count, float* out_c,
                       void* stream);

/*
 * dcts_energy_f32 for `count` tensors of the SAME tile shape (H, W) in one launch (chunks of 32):
 * the single-sweep harness scores every hooked tensor of a shape at the end of the forward pass,
 * and CIFAR-sized layers are too small to fill the GPU one launch at a time. Rows must be dense
 * (strideH == W, strideW == 1). `items` is a HOST array, copied into the kernel arguments.
 * Shapes without a codelet kernel are processed tensor by tensor (same result, no batching);
 * `workspace` must then cover the largest item (dcts_workspace_bytes).
 */
typedef struct dcts_tensor_item {
  const float* x;   /* [N, C_total, H, W] view: element (n,c,h,w) at x[n*strideN + c*strideC + h*W + w] */
  float* out_nc;    /* [N, c_count] */
  int64_t N, C_total, strideN, strideC;
  int32_t c_begin, c_count;
} dcts_tensor_item;
int dcts_energy_multi_f32(const dcts_tensor_item* items, int32_t count, int64_t H, int64_t W,
                          int32_t pad_front_if_odd, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same for tensors of DIFFERENT tile shapes: every hooked tensor of a forward pass in one call.
 * Tensors with square tiles of edge 2, 4, 8, 16 or 32 (every hook point of the reference's CIFAR nets:
 * VGG-16-bn, ResNet-56/110, DenseNet-40, GoogLeNet) share ONE launch per 48 of them, whatever their
 * shapes; the others are grouped by shape as dcts_energy_multi_f32 does. Results are those of one
 * dcts_energy_f32 call per tensor, bit for bit. `workspace` must cover the largest item that needs one.
 */
typedef struct dcts_shaped_item {
  dcts_tensor_item t;
  int64_t H, W;
  int32_t pad_front_if_odd;
  int32_t reserved;
} dcts_shaped_item;
int dcts_energy_mixed_f32(const dcts_shaped_item* items, int32_t count, void* workspace, size_t workspace_bytes,
                          void* stream);

/*
 * Device-side form of the running-mean update of get_feature_hook, utils/common.py:273-277:
 *   c = sum_n energy_nc[n, :]
 *   feature_result = (feature_result * total_before + c) / (total_before + N)
 * feature_result is [C_count] fp32 in/out on the device (zeros before the first batch, like
 * the reference's torch.tensor(0.) broadcast); the caller keeps `total` on the host and
 * adds N after each call. Same three fp32 roundings as the reference (no FMA contraction);
 * the batch sum is the 16-slice fixed-order sum of dcts_batch_sum_f32.
 */
int dcts_running_mean_update_f32(const float* energy_nc, int64_t N, int64_t C_count,
                                 float* feature_result, float total_before, void* stream);

/*
 * The same update for `count` hook points in ONE launch (single-sweep harness: every layer's
 * energies of a batch are ready when the forward pass ends). `descs` is a HOST array; it is
 * copied into the kernel arguments, so it may be reused as soon as the call returns.
 * Every descriptor is checked before anything is enqueued: a negative return leaves every
 * feature_result untouched, so the caller may keep its totals and repeat the batch. Two
 * descriptors of one call must not share a feature_result (their updates are not ordered).
 */
typedef struct dcts_update_desc {
  const float* energy_nc; /* [N, C_count] device */
  float* feature_result;  /* [C_count] device, in/out */
  int64_t N;
  int64_t C_count;
  float total_before;     /* samples accumulated so far for this hook point */
  int32_t reserved;
} dcts_update_desc;
int dcts_running_mean_update_multi_f32(const dcts_update_desc* descs, int32_t count, void* stream);

/*
 * Second scoring criterion (HRank; the reference keeps it as a commented alternative, utils/common.py:268):
 *   out_nc[n*c_count + j] = numerical rank of x[n, c_begin+j], as an exact fp32 integer (all-zero map: +0.0):
 *   the number of singular values sigma_i > max(H, W) * 2^-23 * sigma_max of the fp32 H x W map - the default
 *   rule of torch.linalg.matrix_rank for fp32. Computed in fp64 from the Gram matrix of the map (rank.hip).
 * Addressing as for dcts_energy_f32 (strideW == 1, strideH >= W; no odd pad). Edges 1 ... DCTS_RANK_MAX_EDGE
 * on each axis; an edge in DCTS_RANK_MAX_EDGE+1 ... DCTS_MAX_EDGE returns DCTS_E_UNSUPPORTED. No workspace,
 * no host-side state; the result of a map does not depend on N, the channel slice or the other maps.
 */
#define DCTS_RANK_MAX_EDGE 64
int dcts_rank_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                  int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                  int32_t c_begin, int32_t c_count, float* out_nc, void* stream);

/*
 * Measurement aid (not on the score path): reads n floats once with the kernels' own access
 * width (one dword per lane, coalesced) and discards them. Used to calibrate the FETCH_SIZE
 * performance counter against a known byte count (tools/pmc_traffic.py).
 */
int dcts_debug_stream_read_f32(const float* x, int64_t n, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCTSCORE_H_ */
