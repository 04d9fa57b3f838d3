/*
 * ska_sdp_hip.h -- C ABI of the MI355X-native predict/invert + calibration
 * hot path (libska_sdp_hip.so, hand-written HIP for gfx950).
 *
 * Every entry point takes DEVICE pointers (plain pointers + sizes + strides,
 * no torch types), an optional hipStream_t passed as void*, and an error
 * buffer.  It returns SDP_HIP_OK or one of the error codes below, which the
 * Python layer maps back onto the reference's exception types
 * (AssertionError / ValueError / RuntimeError).
 *
 * Outputs are always caller-allocated (the ska-sdp-func convention of
 * dft_point_v00, reference src/ska_sdp_func_python/imaging/dft.py:169-178);
 * the library never returns memory it allocated.  Internal scratch
 * (visibility records, w-plane grids, FFT plans) lives in a per-device cache
 * that grows on demand and is released by sdp_hip_release_workspace().
 */
#ifndef SKA_SDP_HIP_H
#define SKA_SDP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define SDP_HIP_OK 0
#define SDP_HIP_ERR_INVALID_ARG 1 /* -> ValueError   */
#define SDP_HIP_ERR_RUNTIME 2     /* -> RuntimeError */
#define SDP_HIP_ERR_NO_DEVICE 3   /* -> RuntimeError */
#define SDP_HIP_ERR_MEMORY 4      /* -> MemoryError  */

/* ---- dtype codes ------------------------------------------------------- */
#define SDP_HIP_F32 1
#define SDP_HIP_F64 2
#define SDP_HIP_C64 3
#define SDP_HIP_C128 4

/* ---- flags for the NUFFT pair ------------------------------------------ */
#define SDP_HIP_FLIP_UW 1u    /* negate u and w on the fly (RASCIL, ng.py:210-213) */
#define SDP_HIP_ACCUMULATE 2u /* add into the output instead of overwriting      */
#define SDP_HIP_BATCH_FIRST 4u /* sdp_hip_ms2dirty_batch: first batch (zero the planes) */
#define SDP_HIP_BATCH_LAST 8u  /* sdp_hip_ms2dirty_batch: last batch (FFT + screens)    */
/* sdp_hip_ms2dirty / _vis: bucket every in-grid visibility (zero weights too,
 * they add exact zeros; info.nvis_used then counts them) and keep the
 * bucketing on the device for following SDP_HIP_REUSE_BUCKETS calls */
#define SDP_HIP_KEEP_BUCKETS 16u
/* sdp_hip_ms2dirty / _vis: reuse the kept bucketing (invert_ng's other
 * polarisations): the same uvw and freq arrays, unchanged, and the same nrow,
 * nchan, image geometry, epsilon, do_wstacking and FLIP_UW as the keeping
 * call; only the visibilities, weights, flags and pol differ.  Only the value
 * pass, gridding and FFT run.  Any other wstack call (or a workspace release)
 * in between drops the kept bucketing: the call then fails with
 * SDP_HIP_ERR_INVALID_ARG. */
#define SDP_HIP_REUSE_BUCKETS 32u
/* epsilon below 1e-7 (the reference's default 1e-12 included) runs the fp64
 * NUFFT: W = ceil(-log10(epsilon/10)) in [9, 16], fp64 taps, records, c128
 * planes, Z2Z FFTs, one-cell buckets (grids whose (first plane, cell)
 * histogram exceeds 2^28 keys are refused).  SDP_HIP_FP32 keeps the fp32
 * NUFFT at its floor instead (W = 8, ~1e-6 relative RMS), as before. */
#define SDP_HIP_FP32 64u
/* sdp_hip_ms2dirty_batch: grid one w slab of the sequence's plane layout.
 * `bounds` then holds 8 doubles: the 6 below, then the slab's first planes
 * [lo, hi) (integers, 0 <= lo < hi; hi is clipped to the layout's first-plane
 * count, which sdp_hip_wstack_layout reports).  Only visibilities whose first
 * w plane lies in the slab are gridded -- the others are skipped (tested
 * before their weights or values are read) -- and only planes lo .. hi + W - 2
 * are held, transformed and screened.  The dirty images of the slabs of one
 * layout sum to the full image (multi-GPU w-slab partition).
 * fp32 NUFFT (epsilon >= 1e-7 or SDP_HIP_FP32) with w-stacking only. */
#define SDP_HIP_W_SLAB 128u
/* sdp_hip_ms2dirty / _vis / sdp_hip_dirty2ms / _vis: use the second set of
 * scratch buffers (planes, records, histograms, FFT plans, auxiliary stream).
 * A caller that alternates it between two streams can have two calls in
 * flight at once -- the next call's bucketing runs while the previous one
 * grids and transforms.  Not with KEEP/REUSE_BUCKETS, the batch flags or
 * W_SLAB. */
#define SDP_HIP_SLOT1 256u

/* Diagnostics filled by the NUFFT entry points (may be NULL). */
typedef struct sdp_hip_wgrid_info {
    int support;          /* ES kernel support W                            */
    double beta;          /* ES kernel shape                                */
    int ngrid_x, ngrid_y; /* oversampled grid (sigma = 2)                   */
    int nplanes;          /* w planes (1 when do_wstacking == 0)            */
    double w0, dw;        /* plane 0 position and spacing (wavelengths)     */
    int64_t nvis_used;    /* visibilities with non-zero weight              */
    int64_t nitems;       /* gridding work items launched                   */
    int plane_chunk;      /* planes resident per pass                       */
    float ms_prep, ms_grid, ms_fft, ms_screen; /* stage times if timing on  */
    int bucket;           /* bucket edge in cells: 1 = one-cell buckets,
                             16 = 16x16-cell buckets sub-sorted by cell
                             (large grids)                                  */
    int grid_launches;    /* (de)gridding kernel launches (one per plane
                             chunk); ms_grid is their summed time           */
    int padded;           /* invert: gridded on cells padded to 4 records
                             (k_grid_mfma_pad; 0: k_grid_mfma)              */
    int fp64;             /* the fp64 NUFFT ran (epsilon < 1e-7)            */
    int tiled;            /* one-cell buckets from the two-level (64x64-cell
                             bin, then cell) LDS-histogram sort             */
    int folded;           /* invert: the visibilities with u < 0 were gridded
                             as their Hermitian mirrors (-u, -v, -w, conj), so
                             the plane passes ran over half the row band
                             (SDP_HIP_HFOLD=0 switches it off)              */
    int layout_reused;    /* invert: the two-level sort's layout (bins, cell
                             bases, pads, work items) was the one kept from
                             the slot's previous invert of the same uvw, freq
                             and geometry: only the value pass, a recount and
                             the final move ran.  nvis_used then counts every
                             in-grid visibility, zero weights included
                             (SDP_HIP_LAYOUT_CACHE=0 switches it off)       */
} sdp_hip_wgrid_info;

/* Library/ABI version and a device probe. */
int sdp_hip_version(void);
int sdp_hip_device_count(int *count, char *errbuf, size_t errbuf_len);
int sdp_hip_release_workspace(char *errbuf, size_t errbuf_len);
/* When non-zero, the NUFFT entry points time their stages with HIP events
 * (adds stream synchronisations; off by default). */
int sdp_hip_set_stage_timing(int enable);

/*
 * sdp_hip_ms2dirty -- replaces ducc0.wgridder.ms2dirty as called by
 * invert_ng (reference src/ska_sdp_func_python/imaging/ng.py:240-256 MFS,
 * :271-287 per channel; double_precision_accumulation=True).
 *
 * dirty[x,y] = sum_{row,chan} wgt * Re{vis * exp(2 pi i (u l_x + v m_y - w (n-1)))} [/n]
 * (ducc0 convention, l_x = (x - nx/2) pixsize_x).
 *
 * uvw      [nrow, 3] f64 metres, row stride uvw_row_stride (elements)
 * freq     [nchan] f64 Hz
 * vis      [nrow, nchan] c64 or c128 (vis_dtype SDP_HIP_C64 / SDP_HIP_C128)
 *          with element strides; NULL means unit visibilities (PSF,
 *          ng.py:231-233)
 * wgt      [nrow, nchan] f32 or f64 (wgt_dtype SDP_HIP_F32 / SDP_HIP_F64; ducc0
 *          takes f64) with element strides; NULL means unit weights.  Samples
 *          of zero weight are skipped (their visibilities are never read)
 * dirty    f64, element (x, y) at dirty[x*dirty_stride_x + y*dirty_stride_y]
 *          (pass strides (1, nx) to receive RASCIL's transposed image)
 * epsilon  requested accuracy: >= 1e-7 the fp32 NUFFT (W = ceil(-log10(eps/10)),
 *          <= 8); below 1e-7 the fp64 NUFFT (W in [9, 16], c128 planes) unless
 *          flags has SDP_HIP_FP32 (fp32 at its floor, W = 8)
 */
int sdp_hip_ms2dirty(const double *uvw, int64_t uvw_row_stride,
                     const double *freq, int nchan, int64_t nrow,
                     const void *vis, int vis_dtype, int64_t vis_row_stride,
                     int64_t vis_chan_stride, const void *wgt, int wgt_dtype,
                     int64_t wgt_row_stride, int64_t wgt_chan_stride,
                     int npix_x, int npix_y, double pixsize_x,
                     double pixsize_y, double epsilon, int do_wstacking,
                     unsigned flags, double *dirty, int64_t dirty_stride_x,
                     int64_t dirty_stride_y, void *stream,
                     sdp_hip_wgrid_info *info, char *errbuf,
                     size_t errbuf_len);

/*
 * sdp_hip_ms2dirty_batch -- sdp_hip_ms2dirty over a sequence of visibility
 * batches that share one w-plane layout and one set of resident uv planes
 * (a band too large for one call, e.g. the 13.4 Gvis of C4 on fewer than 8
 * GPUs, streamed through the device channel block by channel block).  Every
 * call of a sequence passes the same image geometry, epsilon, do_wstacking,
 * FLIP_UW and `bounds`; the first carries SDP_HIP_BATCH_FIRST (planes
 * zeroed), the last SDP_HIP_BATCH_LAST (FFT, w-screens, grid correction into
 * `dirty`, which may be NULL before).  The result equals one sdp_hip_ms2dirty
 * call over all batches with that plane layout.
 * bounds   host {min w, max w, max|u|, max|v|} over ALL batches in metres
 *          (uvw as given, before FLIP_UW) and {min freq, max freq} over all
 *          batches' frequencies (6 doubles)
 * Replaces the reference's per-(pol, chan) ducc0 loop as a streaming form of
 * ms2dirty (ng.py:259-289); the planes must all fit on the device.  A batch
 * whose visibilities fall outside `bounds` fails with SDP_HIP_ERR_INVALID_ARG,
 * and so does a later batch when its sequence's planes are gone (another
 * NUFFT call or a workspace release after the first batch) or its geometry,
 * epsilon, flags or bounds differ from the first batch's.
 */
int sdp_hip_ms2dirty_batch(const double *uvw, int64_t uvw_row_stride,
                           const double *freq, int nchan, int64_t nrow,
                           const void *vis, int vis_dtype,
                           int64_t vis_row_stride, int64_t vis_chan_stride,
                           const void *wgt, int wgt_dtype, int64_t wgt_row_stride,
                           int64_t wgt_chan_stride, int npix_x, int npix_y,
                           double pixsize_x, double pixsize_y, double epsilon,
                           int do_wstacking, unsigned flags,
                           const double *bounds, double *dirty,
                           int64_t dirty_stride_x, int64_t dirty_stride_y,
                           void *stream, sdp_hip_wgrid_info *info,
                           char *errbuf, size_t errbuf_len);

/*
 * sdp_hip_wstack_layout -- the w-plane layout sdp_hip_ms2dirty_batch uses for
 * `bounds` (6 doubles, as above) and the image geometry, without device work:
 * info->support, nplanes (first planes = nplanes - support + 1), w0, dw,
 * ngrid_x/y, fp64.  A w-slab partition (SDP_HIP_W_SLAB) splits the first
 * planes [0, nplanes - support + 1) between the ranks.
 */
int sdp_hip_wstack_layout(const double *bounds, int npix_x, int npix_y,
                          double pixsize_x, double pixsize_y, double epsilon,
                          int do_wstacking, unsigned flags, sdp_hip_wgrid_info *info,
                          char *errbuf, size_t errbuf_len);

/*
 * sdp_hip_wstack_fingerprint -- the content fingerprint under which an invert
 * keeps its bucketing layout (info.layout_reused), computed on the host from
 * HOST arrays (no device work; the device computes the same words during the
 * invert's bounds pass).  out = {uvw a, uvw b, freq a, freq b}: per array two
 * 64-bit wrapping sums over its elements of a mix of (index, bit patterns) --
 * independent of the order of summation, not of the order of the content.
 */
int sdp_hip_wstack_fingerprint(const double *uvw, int64_t uvw_row_stride, int64_t nrow,
                               const double *freq, int nchan, uint64_t *out,
                               char *errbuf, size_t errbuf_len);

/*
 * sdp_hip_ms2dirty_vis -- sdp_hip_ms2dirty with the visibility-side prologue
 * of invert_ng fused into its first pass, so the
 * Visibility's own arrays are read in place:
 *   flagged_vis / flagged_imaging_weight (reference imaging/ng.py:191, :202;
 *   value * (1 - flags)), convert_pol_frame (ng.py:193-198) and the weight sum
 *   sumwt (ng.py:258, :289).
 * vis       [nrow, nchan, npol_vis] c64/c128 at pol 0, element strides
 *           (row, chan, pol); NULL = unit visibilities (PSF)
 * pol_coeff host array of 2*npol_vis doubles (re, im): image-pol visibility =
 *           sum_k coeff_k * vis_k * (1 - flag_k) (one row of the conversion
 *           matrix); NULL = no conversion, the image pol is vis pol `pol`
 * wgt       weights of image pol `pol` (f32 or f64, wgt_dtype), strides
 *           (row, chan); NULL = ones
 * vis_flags [nrow, nchan, npol_vis] integers of flag_bytes at pol 0 with
 *           strides, or NULL; the weight is masked with flag pol `pol`
 * sumwt     device double, += sum over rows and channels of the masked
 *           weights (NULL: not computed)
 * shift_lmn host array (l, m, n-1) of the image phase centre relative to the
 *           visibility phase centre, or NULL: shift_vis_to_image's tangent
 *           phase rotation (reference imaging/base.py:48-92,
 *           visibility/base.py:27-90) applied on the fly, vis *
 *           exp(+2 pi i uvw_lambda . lmn) (uvw as given, before FLIP_UW)
 * Other arguments as sdp_hip_ms2dirty.
 */
int sdp_hip_ms2dirty_vis(const double *uvw, int64_t uvw_row_stride,
                         const double *freq, int nchan, int64_t nrow,
                         const void *vis, int vis_dtype, int64_t vis_row_stride,
                         int64_t vis_chan_stride, int64_t vis_pol_stride,
                         int npol_vis, const double *pol_coeff, const void *wgt,
                         int wgt_dtype, int64_t wgt_row_stride,
                         int64_t wgt_chan_stride, const void *vis_flags,
                         int flag_bytes, int64_t flag_row_stride,
                         int64_t flag_chan_stride, int64_t flag_pol_stride,
                         int pol, int npix_x, int npix_y, double pixsize_x,
                         double pixsize_y, double epsilon, int do_wstacking,
                         unsigned flags, double *dirty, int64_t dirty_stride_x,
                         int64_t dirty_stride_y, double *sumwt,
                         const double *shift_lmn, void *stream,
                         sdp_hip_wgrid_info *info, char *errbuf,
                         size_t errbuf_len);

/*
 * sdp_hip_ms2dirty_vis_batch -- sdp_hip_ms2dirty_vis as one batch of a
 * sequence (SDP_HIP_BATCH_FIRST / _LAST in `flags`, `bounds` as
 * sdp_hip_ms2dirty_batch): invert_ng grids an MFS image's (or a cube
 * channel's) visibilities in channel batches through one set of resident w
 * planes when they are too many for one call (reference imaging/ng.py:
 * 240-256, one ducc0 call over all channels).  sumwt accumulates over the
 * batches.  Other arguments as sdp_hip_ms2dirty_vis.
 */
int sdp_hip_ms2dirty_vis_batch(const double *uvw, int64_t uvw_row_stride,
                               const double *freq, int nchan, int64_t nrow,
                               const void *vis, int vis_dtype, int64_t vis_row_stride,
                               int64_t vis_chan_stride, int64_t vis_pol_stride,
                               int npol_vis, const double *pol_coeff, const void *wgt,
                               int wgt_dtype, int64_t wgt_row_stride,
                               int64_t wgt_chan_stride, const void *vis_flags,
                               int flag_bytes, int64_t flag_row_stride,
                               int64_t flag_chan_stride, int64_t flag_pol_stride,
                               int pol, int npix_x, int npix_y, double pixsize_x,
                               double pixsize_y, double epsilon, int do_wstacking,
                               unsigned flags, const double *bounds, double *dirty,
                               int64_t dirty_stride_x, int64_t dirty_stride_y,
                               double *sumwt, const double *shift_lmn, void *stream,
                               sdp_hip_wgrid_info *info, char *errbuf,
                               size_t errbuf_len);

/*
 * sdp_hip_ms2dirty_vis_pols -- every image pol of one invert_ng image channel
 * in one call (reference imaging/ng.py:240-289: one ducc0 ms2dirty per image
 * pol over the same uvw).  The pols share one bucketing, and one value pass
 * reads each visibility's pols, flags and weights once and writes every
 * pol's records; then each pol is gridded, transformed and screened into its
 * own image.  Results as npol_img sdp_hip_ms2dirty_vis calls, pol q with row
 * q of the conversion matrix, the weights and flag mask of pol q.
 * pol_coeff host array of 2*npol_img*npol_vis doubles: row q, vis pol k at
 *           2*(q*npol_vis+k) (re, im); NULL = identity (image pol q = vis pol q)
 * wgt       weights [nrow, nchan, >= npol_img] (f32 or f64), strides (row,
 *           chan, pol); required
 * dirty     image pol q at dirty + q*dirty_stride_pol, strides (x, y)
 * sumwt     device doubles, pol q at sumwt + q*sumwt_stride (+= its masked
 *           weight sum), or NULL
 * npol_img  1..npol_vis.  flags may not hold KEEP / REUSE / BATCH bits.
 * fp64 plans (epsilon < 1e-7 without SDP_HIP_FP32) and plans outside the
 * one-cell single-level bucketing run the pols as separate calls.
 * Other arguments as sdp_hip_ms2dirty_vis.
 */
int sdp_hip_ms2dirty_vis_pols(const double *uvw, int64_t uvw_row_stride,
                              const double *freq, int nchan, int64_t nrow,
                              const void *vis, int vis_dtype, int64_t vis_row_stride,
                              int64_t vis_chan_stride, int64_t vis_pol_stride,
                              int npol_vis, const double *pol_coeff, int npol_img,
                              const void *wgt, int wgt_dtype, int64_t wgt_row_stride,
                              int64_t wgt_chan_stride, int64_t wgt_pol_stride,
                              const void *vis_flags, int flag_bytes,
                              int64_t flag_row_stride, int64_t flag_chan_stride,
                              int64_t flag_pol_stride, int npix_x, int npix_y,
                              double pixsize_x, double pixsize_y, double epsilon,
                              int do_wstacking, unsigned flags, double *dirty,
                              int64_t dirty_stride_x, int64_t dirty_stride_y,
                              int64_t dirty_stride_pol, double *sumwt,
                              int64_t sumwt_stride, const double *shift_lmn,
                              void *stream, sdp_hip_wgrid_info *info, char *errbuf,
                              size_t errbuf_len);

/*
 * sdp_hip_dirty2ms -- replaces ducc0.wgridder.dirty2ms as called by
 * predict_ng (reference src/ska_sdp_func_python/imaging/ng.py:99-112 MFS,
 * :117-129 per channel).  Exact adjoint of sdp_hip_ms2dirty:
 * vis = wgt * sum_{x,y} dirty[x,y] exp(-2 pi i (u l_x + v m_y - w (n-1))) [/n]
 */
int sdp_hip_dirty2ms(const double *uvw, int64_t uvw_row_stride,
                     const double *freq, int nchan, int64_t nrow,
                     const double *dirty, int64_t dirty_stride_x,
                     int64_t dirty_stride_y, int npix_x, int npix_y,
                     double pixsize_x, double pixsize_y, const void *wgt,
                     int wgt_dtype, int64_t wgt_row_stride, int64_t wgt_chan_stride,
                     double epsilon, int do_wstacking, unsigned flags,
                     void *vis, int vis_dtype, int64_t vis_row_stride,
                     int64_t vis_chan_stride, void *stream,
                     sdp_hip_wgrid_info *info, char *errbuf,
                     size_t errbuf_len);

/*
 * sdp_hip_dirty2ms_vis -- sdp_hip_dirty2ms for ONE image pol of predict_ng
 * with the image -> visibility pol-frame conversion (reference
 * imaging/ng.py:131-136) fused into the write-back: every output pol k of
 * vis [nrow, nchan, npol_vis] (element strides row, chan, pol; vis points at
 * pol 0) receives coeff_k * (this pol's predicted visibility), coeff_k =
 * column `pol` of the conversion matrix, host array of 2*npol_vis doubles
 * (NULL: output pol 0 only).  Without SDP_HIP_ACCUMULATE all npol_vis pols
 * are overwritten (zero where nothing is predicted); call the first image pol
 * without and the others with SDP_HIP_ACCUMULATE.  No weights (predict_ng
 * passes none, ng.py:99-129).  shift_lmn (host (l, m, n-1) or NULL) applies
 * shift_vis_to_image(inverse=True): vis * exp(-2 pi i uvw_lambda . lmn).
 */
int sdp_hip_dirty2ms_vis(const double *uvw, int64_t uvw_row_stride,
                         const double *freq, int nchan, int64_t nrow,
                         const double *dirty, int64_t dirty_stride_x,
                         int64_t dirty_stride_y, int npix_x, int npix_y,
                         double pixsize_x, double pixsize_y, double epsilon,
                         int do_wstacking, unsigned flags, void *vis,
                         int vis_dtype, int64_t vis_row_stride,
                         int64_t vis_chan_stride, int64_t vis_pol_stride,
                         int npol_vis, const double *pol_coeff,
                         const double *shift_lmn, void *stream,
                         sdp_hip_wgrid_info *info, char *errbuf,
                         size_t errbuf_len);

/*
 * sdp_hip_dirty2ms_vis_pols -- every image pol of one predict_ng MFS call in
 * one call (reference imaging/ng.py:99-112 per image pol, :131-136 the pol
 * conversion): the pols share one bucketing; each image pol's planes are
 * built and degridded, and one write-back combines all pols into every
 * visibility pol.  Results as npol_img sdp_hip_dirty2ms_vis calls, the first
 * without and the others with SDP_HIP_ACCUMULATE, pol q with column q of the
 * conversion matrix.
 * dirty     image pol q at dirty + q*dirty_stride_pol, strides (x, y)
 * pol_coeff host array of 2*npol_img*npol_vis doubles: image pol q, vis pol k
 *           at 2*(q*npol_vis+k) (re, im); NULL = identity
 * Other arguments as sdp_hip_dirty2ms_vis.
 */
int sdp_hip_dirty2ms_vis_pols(const double *uvw, int64_t uvw_row_stride,
                              const double *freq, int nchan, int64_t nrow,
                              const double *dirty, int64_t dirty_stride_x,
                              int64_t dirty_stride_y, int64_t dirty_stride_pol,
                              int npol_img, int npix_x, int npix_y, double pixsize_x,
                              double pixsize_y, double epsilon, int do_wstacking,
                              unsigned flags, void *vis, int vis_dtype,
                              int64_t vis_row_stride, int64_t vis_chan_stride,
                              int64_t vis_pol_stride, int npol_vis,
                              const double *pol_coeff, const double *shift_lmn,
                              void *stream, sdp_hip_wgrid_info *info, char *errbuf,
                              size_t errbuf_len);

/*
 * sdp_hip_dft_point_v00 -- replaces ska_sdp_func.visibility.dft_point_v00
 * (reference src/ska_sdp_func_python/imaging/dft.py:173-178) and the cupy
 * dft_kernel (:185-262, :288-337).  Caller-allocated output, replaced (not
 * accumulated), all arrays C-contiguous:
 *   direction_cosines [ncomp, 3] f64 (l, m, n-1)
 *   fluxes            [ncomp, flux_nchan, npol] c128; flux_nchan == nchan
 *                     or 1 (broadcast over channels, as numpy does in
 *                     dft_cpu_looped, dft.py:284)
 *   uvw_lambda        [ntimes*nbaselines, nchan, 3] f64 wavelengths
 *   vis               [ntimes*nbaselines, nchan, npol] c64 or c128
 * vis = sum_c flux[c] * exp(-2 pi i (u l + v m + w (n-1)))   (no 1/n)
 */
int sdp_hip_dft_point_v00(int ncomp, const double *direction_cosines,
                          const void *fluxes, int flux_nchan, int npol,
                          int64_t nrow, int nchan, const double *uvw_lambda,
                          void *vis, int vis_dtype, void *stream,
                          char *errbuf, size_t errbuf_len);

/* Same contraction with uvw in metres [nrow, 3] + freq [nchan]: the lambda
 * scaling (reference visibility/base.py:54-56) is fused into the kernel so
 * the [nrow, nchan, 3] uvw_lambda array is never materialised. */
int sdp_hip_dft_point_metres(int ncomp, const double *direction_cosines,
                             const void *fluxes, int flux_nchan, int npol,
                             int64_t nrow, int nchan, const double *uvw,
                             const double *freq, void *vis, int vis_dtype,
                             void *stream, char *errbuf, size_t errbuf_len);

/*
 * sdp_hip_idft_point_v00 -- the adjoint of sdp_hip_dft_point_v00: the two
 * sums of idft_visibility_skycomponent (reference
 * src/ska_sdp_func_python/imaging/dft.py:340-387; flux :365-370, weight
 * :371, phasor visibility/base.py:27-45) for all components in one call.
 * Caller-allocated outputs, replaced (not accumulated), all arrays
 * C-contiguous:
 *   direction_cosines [ncomp, 3] f64 (l, m, n-1)
 *   uvw_lambda        [ntimes*nbaselines, nchan, 3] f64 wavelengths
 *   vis               [ntimes*nbaselines, nchan, npol] c64 or c128
 *   weight            [ntimes*nbaselines, nchan, npol] f64
 *   flags             [ntimes*nbaselines, nchan, npol] 0/1 integers of
 *                     flag_bytes (1, 4 or 8) bytes, or NULL (none flagged)
 *   flux_sum          [ncomp, nchan, npol] c128
 *   sumwt             [nchan, npol] f64, or NULL (not wanted)
 * flux_sum = sum_row weight (1 - flag) vis exp(+2 pi i (u l + v m + w (n-1)))
 * sumwt    = sum_row weight (1 - flag)
 * Both are UNNORMALISED: the reference's flux is flux_sum / sumwt where
 * sumwt > 0 and 0 elsewhere (:373-374), left to the caller so that row shards
 * can be summed first.  complex128 vis: fp64 sincos, products and sums;
 * complex64 vis: fp32 sincos and products, fp32 partial sums of at most 32
 * terms added into fp64.  No atomics: the same inputs give the same bits.
 * nrow == 0 writes zeros; ncomp == 0 writes only sumwt; npol must be 1, 2 or
 * 4 (SDP_HIP_ERR_INVALID_ARG otherwise).
 */
int sdp_hip_idft_point_v00(int ncomp, const double *direction_cosines, int npol,
                           int64_t nrow, int nchan, const double *uvw_lambda,
                           const void *vis, int vis_dtype, const double *weight,
                           const void *flags, int flag_bytes, void *flux_sum,
                           double *sumwt, void *stream, char *errbuf,
                           size_t errbuf_len);

/* Same sums with uvw in metres [nrow, 3] + freq [nchan]: the lambda scaling
 * (reference visibility/base.py:54-56) is fused into the kernel so the
 * [nrow, nchan, 3] uvw_lambda array is never materialised. */
int sdp_hip_idft_point_metres(int ncomp, const double *direction_cosines, int npol,
                              int64_t nrow, int nchan, const double *uvw,
                              const double *freq, const void *vis, int vis_dtype,
                              const double *weight, const void *flags,
                              int flag_bytes, void *flux_sum, double *sumwt,
                              void *stream, char *errbuf, size_t errbuf_len);

/*
 * Convolution-function (AW-projection) gridder/degridder, replacing the
 * Python triple loops of grid_visibility_to_griddata /
 * degrid_visibility_from_griddata (reference
 * src/ska_sdp_func_python/grid_data/gridding.py:160-255, :502-590).
 * The Python layer evaluates the reference's WCS mappings
 * (spatial_mapping, gridding.py:60-157) into integer indices; the kernels do
 * the per-visibility slice add / einsum, including the edge-skip rule
 * (gridding.py:230-237).
 *   pu,pv,pwc,pdu,pdv [nchan_vis, nrowvis] int32 (per channel mappings)
 *   vis,wt            [nrowvis, nchan_vis, npol] c128 / f64 (flagged)
 *   cf                [cf_nchan, npol, nw, ndv, ndu, gv, gu] c128
 *   grid              [g_nchan, npol, ny, nx] c128 (accumulated)
 *   vis_to_im         [nchan_vis] int32
 *   sumwt             [g_nchan, npol] f64 (accumulated)
 *   nskipped          [1] int64 (accumulated count of edge-skipped rows)
 */
int sdp_hip_grid_cf(int64_t nrowvis, int nchan_vis, int npol,
                    const int32_t *pu, const int32_t *pv, const int32_t *pwc,
                    const int32_t *pdu, const int32_t *pdv,
                    const int32_t *vis_to_im, const void *vis,
                    const double *wt, const void *cf, int cf_nchan, int nw,
                    int ndv, int ndu, int gv, int gu, void *grid,
                    int g_nchan, int ny, int nx, double *sumwt,
                    int64_t *nskipped, void *stream, char *errbuf,
                    size_t errbuf_len);
int sdp_hip_degrid_cf(int64_t nrowvis, int nchan_vis, int npol,
                      const int32_t *pu, const int32_t *pv,
                      const int32_t *pwc, const int32_t *pdu,
                      const int32_t *pdv, const int32_t *vis_to_im,
                      const void *grid, int g_nchan, int ny, int nx,
                      const void *cf, int cf_nchan, int nw, int ndv, int ndu,
                      int gv, int gu, void *vis_out, int64_t *nskipped,
                      void *stream, char *errbuf, size_t errbuf_len);

/*
 * Batched iterative-substitution gain solver, replacing
 * _solve_with_mask + _solve_antenna_gains_itsubs_scalar / _matrix /
 * _nocrossdata + the residual functions (reference
 * src/ska_sdp_func_python/calibration/solvers.py:148-539).  One solve = one
 * gain-table row; all of its channels (and 2x2 components) iterate together
 * and stop on max|g - g_last| over antennas AND channels (solvers.py:268,
 * :427), as in the reference.
 *   baselines   canonical: a1 < a2, sorted by (a1, a2); row_start[nants+1]
 *               is the CSR offset of each a1, ant2[nbl] the partner
 *   xb, wb      [nsolve, nbl, nchan, npol] c128 / f64: the weighted sums
 *               sum(V w) and sum(w) of solvers.py:99-107 (point-source vis)
 *   gain        [nsolve, nants, nchan, nrec, nrec] c128 (in: start, out)
 *   gwt         [nsolve, nants, nchan, nrec, nrec] f64   (out)
 *   residual    [nsolve, nchan, nrec, nrec] f64          (out)
 *   niter_out   [nsolve] int32 iterations used (niter + 1: not converged)
 * mode: 0 scalar (npol 1), 1 matrix (npol 4, crosspol), 2 no cross data
 * (npol 2, or npol 4 without crosspol).
 */
int sdp_hip_solve_gains(int nsolve, int nants, int nbl, const int32_t *row_start,
                        const int32_t *ant2, int nchan, int npol, int mode,
                        const void *xb, const double *wb, void *gain, double *gwt,
                        double *residual, int32_t *niter_out, int niter, double tol,
                        int phase_only, int refant, double damping, void *stream,
                        char *errbuf, size_t errbuf_len);

/*
 * Calibration neighbours of StefCal.  Visibility
 * arrays are the Visibility's [ntimes, nbl, nchan, npol] in C order:
 * vis / model c64 or c128 (vis_dtype), weight f64, flags integers of
 * flag_bytes (1, 4, 8) or NULL; model_flags (same type) masks the model
 * where the model Visibility carries flags of its own (NULL: the vis flags).
 *
 * sdp_hip_point_sums: divide_visibility (reference
 * src/ska_sdp_func_python/visibility/operations.py:145-189; model may be
 * NULL = no division) fused with solve_gaintable's per-gain-row sums
 * (calibration/solvers.py:82-107):
 *   x_b[r, j, fg, p]  = sum_{t in row r} sum_{f} x * xwt * (1 - flag)
 *   xwt_b[r, j, fg, p] = sum ... xwt * (1 - flag)
 * over all channels f when nchan_g == 1, else f = fg.  Row r's vis time
 * indices are time_idx[row_ptr[r] .. row_ptr[r+1]) (device int32 CSR).
 * Output baseline j < nbl_out reads source baseline bl_perm[j] (NULL =
 * identity, nbl_out = nbl) and is conjugated where bl_conj[j] (NULL = never):
 * StefCal's canonical order.  xb c128 / xwt f64 [nrow_g, nbl_out, nchan_g,
 * npol], overwritten.
 */
int sdp_hip_point_sums(int64_t ntimes, int nbl, int nchan, int npol,
                       const void *vis, const void *model, int vis_dtype,
                       const double *weight, const void *flags,
                       const void *model_flags, int flag_bytes,
                       int nrow_g, const int32_t *row_ptr,
                       const int32_t *time_idx, int nchan_g, int nbl_out,
                       const int32_t *bl_perm, const uint8_t *bl_conj, void *xb,
                       double *xwt, void *stream, char *errbuf,
                       size_t errbuf_len);
/* divide_visibility alone over n samples: x_out = fv / fm where
 * xwt_out = |fm|^2 fw > 0, else 0 (f = flagged); x_out has vis_dtype. */
int sdp_hip_divide_vis(int64_t n, const void *vis, const void *model,
                       int vis_dtype, const double *weight, const void *flags,
                       const void *model_flags, int flag_bytes, void *x_out,
                       double *xwt_out, void *stream, char *errbuf,
                       size_t errbuf_len);
/*
 * sdp_hip_apply_gains: apply_gaintable (calibration/operations.py:23-256) in
 * place on vis / weight.  time_row[ntimes] (device int32) is the gain row
 * applied to each vis time, or -1; ant1/ant2 [nbl] int32 the baseline's
 * antennas; gain c128 [nrow_g, nants, nchan_g, nrec, nrec].  Gain channel c
 * acts on vis channel c only (channels >= nchan_g keep their values, as in
 * the reference).  npol 1: V * sum_lm g1 conj(g2) (1/g where |g| > 0 for
 * inverse), zero vis + weight where that is 0; npol 2 / 4: G1 V conj(G2)
 * (elementwise conj) with V diagonal / 2x2, inverse = the 2x2 inverses; a
 * baseline with a singular gain zeroes pol 0 (npol 2) or all pols (npol 4)
 * and their weights.  use_flags: a gain row whose window holds any set flag
 * works on the flagged vis / weights of that window.
 */
int sdp_hip_apply_gains(int64_t ntimes, int nbl, int nchan, int npol,
                        void *vis, int vis_dtype, double *weight,
                        const void *flags, int flag_bytes, int use_flags,
                        const int32_t *ant1, const int32_t *ant2,
                        const int32_t *time_row, const void *gain, int nrow_g,
                        int nants, int nchan_g, int nrec, int inverse,
                        void *stream, char *errbuf, size_t errbuf_len);
/*
 * sdp_hip_apply_gain_chain: the gain tables of apply_calibration_chain
 * (calibration/chain_calibration.py:75-134) applied in the given order in ONE
 * pass over vis / weight (in place), bit for bit what ntab calls of
 * sdp_hip_apply_gains with use_flags = 0 give: an element stays in registers,
 * and a complex64 value is rounded to float between two tables as a store
 * and reload would round it; weights stay f64.  1 <= ntab <=
 * SDP_HIP_GAIN_CHAIN_MAX (longer chains: consecutive calls).  gains and
 * time_rows are HOST arrays of ntab device pointers: table k has gains c128
 * [nrow_g[k], nants, nchan_g[k], nrec[k], nrec[k]] and its own time_row map
 * [ntimes] (device int32, -1 = no row of table k owns this time); nrow_g,
 * nchan_g, nrec are host int32 [ntab].  One inverse flag for the whole chain.
 * An element whose time no table covers is not written.  Refused: ntab outside
 * the range, nrec not 1 or 2, npol 2 or 4 with nrec 1, null pointers.
 */
#define SDP_HIP_GAIN_CHAIN_MAX 8
int sdp_hip_apply_gain_chain(int64_t ntimes, int nbl, int nchan, int npol,
                             void *vis, int vis_dtype, double *weight,
                             const int32_t *ant1, const int32_t *ant2,
                             int nants, int ntab, const void *const *gains,
                             const int32_t *const *time_rows,
                             const int32_t *nrow_g, const int32_t *nchan_g,
                             const int32_t *nrec, int inverse, void *stream,
                             char *errbuf, size_t errbuf_len);

/*
 * Imaging weights, replacing the Python row loops of
 * grid_visibility_weight_to_griddata (reference
 * src/ska_sdp_func_python/grid_data/gridding.py:258-334) and
 * griddata_visibility_reweight (:362-499), which weight_visibility
 * (src/ska_sdp_func_python/imaging/weighting.py:35-68) chains, and the two
 * tapers (weighting.py:71-136).
 *   uvw          [nrow, 3] f64 metres (nrow = ntimes * nbaselines)
 *   freq         [nchan] f64 Hz
 *   weight       [nrow, nchan, npol] f64 (the Visibility's weight)
 *   flags        [nrow, nchan, npol] integers of flag_bytes (1, 4 or 8) or
 *                NULL; flagged weight = weight * (1 - flags) as in the
 *                datamodels' flagged_weight
 *   vis_to_im    [nchan] int32 image channel of each visibility channel
 *   grid_wcs     [6] f64: crval, cdelt, crpix of the GridData's UU axis, then
 *                of its VV axis; cell = round((uv - crval) / cdelt + crpix - 1)
 *   grid         [g_nchan, npol, ny, nx] f64: real part of the GridData
 *   npol         1, 2 or 4
 */
/* Accumulates the flagged weight into grid at the sample's cell and at its
 * conjugate's; sumwt [g_nchan, npol] += 2 * weight; rows whose cell or
 * conjugate cell is off the grid add npol to *nskipped (int64, accumulated). */
int sdp_hip_grid_weights(int64_t nrow, int nchan, int npol, const double *uvw,
                         const double *freq, const double *weight,
                         const void *flags, int flag_bytes,
                         const int32_t *vis_to_im, const double *grid_wcs,
                         double *grid, int g_nchan, int ny, int nx,
                         double *sumwt, int64_t *nskipped, void *stream,
                         char *errbuf, size_t errbuf_len);
/* weighting 0 natural (imaging_weight = weight), 1 uniform (flagged weight /
 * grid weight), 2 robust (flagged weight / (1 + f2 * grid weight), f2 =
 * robust_coef * sum(sumwt) / sum(grid^2), robust_coef = (5 * 10^-robustness)^2;
 * sumwt NULL means 2 * sum of flagged weights).  imaging_weight
 * [nrow, nchan, npol] f64 is overwritten (it is read only where the grid
 * weight is NaN, as the reference keeps the flagged imaging weight there). */
int sdp_hip_reweight(int64_t nrow, int nchan, int npol, const double *uvw,
                     const double *freq, const double *weight,
                     const void *flags, int flag_bytes,
                     const int32_t *vis_to_im, const double *grid_wcs,
                     const double *grid, int g_nchan, int ny, int nx,
                     int weighting, double robust_coef, const double *sumwt,
                     int n_sumwt, double *imaging_weight, void *stream,
                     char *errbuf, size_t errbuf_len);
/* imaging_weight = flagged imaging weight * taper(row, chan), in place.
 * kind 0 gaussian: exp(-param * |uv|^2 / lambda^2), param = pi^2 beam^2 / (4 ln 2);
 * kind 1 tukey: tukey_filter(|uv| / max|uv|, param). */
int sdp_hip_taper(int64_t nrow, int nchan, int npol, const double *uvw,
                  const double *freq, const void *flags, int flag_bytes,
                  int kind, double param, double *imaging_weight, void *stream,
                  char *errbuf, size_t errbuf_len);

/*
 * CLEAN minor cycles on one image plane, replacing the numpy loops of the
 * reference's hogbom (src/ska_sdp_func_python/image/cleaners.py:23-133) and
 * msclean (:403-452, with find_max_abs_stack :565-610).  Everything is fp64
 * and evaluated in the reference's order without contraction.
 *   res            [nscales, ny, nx], updated in place: the residual (hogbom,
 *                  nscales 1) or the scale-convolved residual stack
 *   psf            [nscales, nscales, psf_ny, psf_nx]: the PSF (hogbom) or
 *                  its scale cross terms; pixel (psf_ny/2, psf_nx/2) lands on
 *                  the peak, the patch is [peak - n/2, peak + n/2) clipped
 *   window         [nscales, ny, nx] or NULL: multiplies the search value
 *   sensitivity    [ny, nx] or NULL (msclean only): the search uses
 *                  resid * sens^2, the comparison across scales resid * sens
 *   coupling_diag  [nscales] host doubles (msclean; NULL for hogbom)
 *   scale_kernels  [nscales, psf_ny, psf_nx] (msclean; NULL for hogbom):
 *                  added into comps, times gain * mval, on the patch
 *   scale_extent   every scale kernel is zero further than this many pixels
 *                  from (psf_ny/2, psf_nx/2), so that only that part of the
 *                  patch is visited for comps; <= 0: the whole patch
 *   comps          [ny, nx], accumulated into
 *   absthresh      max(thresh, fracthresh * max|.|); cycles stop below
 *                  0.9 * absthresh (hogbom: tested after the subtraction and
 *                  that cycle counts; msclean: before, and on mval == 0)
 * The peak is the first maximum in row-major order, the lower scale on a tie.
 * *niter_done is the reference's iteration count, *stop_reason one of
 * SDP_HIP_CLEAN_STOP_*.  The call returns after the last cycle has run.
 */
#define SDP_HIP_CLEAN_HOGBOM 0
#define SDP_HIP_CLEAN_MSCLEAN 1
#define SDP_HIP_CLEAN_STOP_NITER 0
#define SDP_HIP_CLEAN_STOP_THRESHOLD 1
#define SDP_HIP_CLEAN_STOP_ZERO 2
int sdp_hip_clean_plane(int algorithm, int nscales, int ny, int nx,
                        int psf_ny, int psf_nx, double *res, const double *psf,
                        const double *window, const double *sensitivity,
                        const double *coupling_diag,
                        const double *scale_kernels, int scale_extent,
                        double *comps, double gain, double pmax,
                        double absthresh, int niter,
                        int *niter_done, int *stop_reason, void *stream,
                        char *errbuf, size_t errbuf_len);

/*
 * Complex Hogbom CLEAN minor cycles of a Stokes Q and a Stokes U plane as
 * P = Q + iU (Pratley & Johnston-Hollitt 2016), replacing the numpy loop of
 * the reference's hogbom_complex (src/ska_sdp_func_python/image/
 * cleaners.py:136-232).  Everything is fp64, contiguous and updated in place.
 *   res      [2, ny, nx]: plane 0 is Q, plane 1 is U
 *   psf      [psf_ny, psf_nx], shared by both planes (>= 2 x 2); pixel
 *            (psf_ny/2, psf_nx/2) lands on the peak, the patch is
 *            [peak - n/2, peak + n/2) clipped to the image
 *   window   [ny, nx] or NULL: multiplies both planes in the search
 *   comps    [2, ny, nx], accumulated into
 *   pmax     the PSF's maximum, > 0 (it need not be 1)
 * One cycle, every step a single IEEE operation without contraction:
 *   search   the key of a pixel is hypot(q * w, u * w) (w = 1 without a
 *            window); the largest key wins, the lower flat index on a tie at
 *            every reduction level; a NaN key is never selected and an
 *            all-NaN plane gives index 0
 *   value    mval_q = (q * gain) * rinv and mval_u = (u * gain) * rinv with
 *            rinv = 1.0 / pmax formed once per call: numpy's division of a
 *            complex scalar by a real one (NOT (q * gain) / pmax)
 *   comps    comps_q[peak] += mval_q, comps_u[peak] += mval_u
 *   residual on the patch q -= psf * mval_q and u -= psf * mval_u, one
 *            multiplication and one subtraction each
 *   stop     after the subtraction, once hypot(q, u) at the peak pixel is
 *            < absthresh -- absthresh itself, not the 0.9 * absthresh of
 *            sdp_hip_clean_plane; that cycle counts
 * *niter_done is the reference's iteration count, *stop_reason
 * SDP_HIP_CLEAN_STOP_NITER or _THRESHOLD.  The call returns after the last
 * cycle has run.
 */
int sdp_hip_clean_plane_complex(int ny, int nx, int psf_ny, int psf_nx,
                                double *res, const double *psf,
                                const double *window, double *comps,
                                double gain, double pmax, double absthresh,
                                int niter, int *niter_done, int *stop_reason,
                                void *stream, char *errbuf, size_t errbuf_len);

/*
 * Multi-scale multi-frequency CLEAN minor cycles on one polarisation (Rau &
 * Cornwell 2011, Algorithm 1), replacing the numpy loop of the reference's
 * msmfsclean (src/ska_sdp_func_python/image/cleaners.py:831-876, with
 * find_global_optimum :901-974, the two updates :977-1031, the principal
 * solution :1107-1121 and find_optimum_scale_zero_moment :1124-1157).
 * Everything is fp64, evaluated without contraction in the left-to-right
 * order numpy's einsum takes.  nscales <= 16, nmoment <= 4.
 *   smresidual     [nscales, nmoment, ny, nx], updated in place
 *   m_model        [nmoment, ny, nx], accumulated into
 *   ssmmpsf        [nscales, nscales, 2 * nmoment - 1, psf_ny, psf_nx]:
 *                  plane k is the reference's ssmmpsf[s, p, t, q] for every
 *                  t + q = k (it stores nmoment^2 copies); pixel
 *                  (psf_ny/2, psf_nx/2) lands on the peak, the patch is
 *                  [peak - n/2, peak + n/2) clipped
 *   scale_kernels  [nscales, psf_ny, psf_nx]: added into every model moment,
 *                  times gain * mval[moment], on the patch
 *   scale_extent   as for sdp_hip_clean_plane
 *   windowstack    [nscales, ny, nx] or NULL
 *   sensitivity    [ny, nx] or NULL
 *   hsmmpsf, ihsmmpsf  [nscales, nmoment, nmoment] host doubles: the Hessian
 *                  of every scale and its inverse
 *   findpeak       SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL: the search field of
 *                  scale s is the principal solution's moment 0 (the
 *                  reference's "RASCIL", "Algorithm1" and anything else);
 *                  _CASA: its dchisq
 *   absthresh      max(thresh, fracthresh * max|smresidual[0, 0]|): a cycle
 *                  whose |mval[0]| is below it is counted and stops, before
 *                  its update
 * Per scale the peak is the first maximum of |field| in row-major order,
 * WITHOUT window or sensitivity; the scales are compared on
 * max|field * window * sensitivity| with a strict '>' from 0 (the lower
 * scale wins a tie; nothing above 0 selects pixel (0, 0) of scale 0).
 * *niter_done is the reference's iteration count, *stop_reason
 * SDP_HIP_CLEAN_STOP_NITER or _THRESHOLD, scale_counts[nscales] (host) the
 * cycles that chose each scale.  The call returns after the last cycle.
 */
#define SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL 0
#define SDP_HIP_MFSCLEAN_FINDPEAK_CASA 1
int sdp_hip_mfsclean_plane(int nscales, int nmoment, int ny, int nx,
                           int psf_ny, int psf_nx, double *smresidual,
                           double *m_model, const double *ssmmpsf,
                           const double *scale_kernels, int scale_extent,
                           const double *windowstack,
                           const double *sensitivity, const double *hsmmpsf,
                           const double *ihsmmpsf, int findpeak, double gain,
                           double absthresh, int niter, int *niter_done,
                           int *stop_reason, int *scale_counts, void *stream,
                           char *errbuf, size_t errbuf_len);

/*
 * Visibility operations (reference src/ska_sdp_func_python/visibility/
 * operations.py).  Arrays are the Visibility's [ntimes, nbl, nchan, npol] in
 * C order with nrows = ntimes * nbl: vis c64 or c128 (vis_dtype), weight and
 * imaging_weight f64, flags integers of flag_bytes (1, 4, 8) or NULL;
 * npol 1, 2 or 4.  Arithmetic is fp64 in numpy's order of operations; a c64
 * result is rounded once on output.
 *
 * sdp_hip_vis_average_channels: integrate_visibility_by_channel (:192-235,
 * variant 0, group == nchan) and average_visibility_by_channel (:238-306,
 * variant 1, every group of `group` channels in one call; group divides
 * nchan).  Outputs [nrows, nchan / group, npol]:
 *   weight_out         = sum of weight (1 - flag) over the group
 *   imaging_weight_out = sum of imaging_weight (1 - flag)
 *   flags_out          = 1 where the group's flag count reaches the TOTAL
 *                        nchan (both reference functions compare with nchan),
 *                        else 0; integers of flags_out_bytes
 *   vis_out            = sum of vis (weight (1 - flag)) [variant 0] or of
 *                        (vis (1 - flag)) weight [variant 1], divided by
 *                        d = weight_out (1 - flags_out) where d > 0 (numpy's
 *                        complex / real division)
 * The sums add the channels in numpy.sum(axis=-2)'s order: one by one for
 * npol 2 and 4, numpy's pairwise order for npol 1; with c128 input the result
 * is numpy's bit for bit.
 */
int sdp_hip_vis_average_channels(int64_t nrows, int nchan, int npol, int group,
                                 int variant, const void *vis, int vis_dtype,
                                 const double *weight,
                                 const double *imaging_weight,
                                 const void *flags, int flag_bytes,
                                 void *vis_out, double *weight_out,
                                 double *imaging_weight_out, void *flags_out,
                                 int flags_out_bytes, void *stream,
                                 char *errbuf, size_t errbuf_len);
/*
 * sdp_hip_vis_to_stokes over nsamples = ntimes * nbl * nchan samples.
 * SDP_HIP_STOKES_IQUV: convert_visibility_to_stokes (:309-333), in place,
 * npol 4: vis <- M vis with matrix (HOST, 16 complex as 32 doubles, row =
 * output pol) and every pol's flag <- flag[0] | flag[3]; the other pointers
 * are unused.  SDP_HIP_STOKES_I: convert_visibility_to_stokesI (:336-420),
 * npol 2 or 4, into [nsamples] outputs, with first = pol 0, last = pol
 * npol - 1 and fv, fw the flagged values:
 *   vis_out = 0.5 (fv[first] + fv[last]),  weight_out = fw[first] + fw[last]
 *   (imaging_weight_out likewise),  flags_out = flag[first] | flag[last]
 */
#define SDP_HIP_STOKES_IQUV 0
#define SDP_HIP_STOKES_I 1
int sdp_hip_vis_to_stokes(int64_t nsamples, int npol, int mode, void *vis,
                          int vis_dtype, const double *weight,
                          const double *imaging_weight, void *flags,
                          int flag_bytes, const double *matrix, void *vis_out,
                          double *weight_out, double *imaging_weight_out,
                          void *flags_out, int flags_out_bytes, void *stream,
                          char *errbuf, size_t errbuf_len);
/*
 * sdp_hip_vis_remove_continuum: remove_continuum_visibility (:108-142), in
 * place.  For each spectrum (row, pol) a polynomial of `degree` (0 to 5) in
 * x[nchan] (device f64, the reference's scaled frequency) is fitted to vis
 * with weights weight (1 - flag), 0 where mask[nchan] (device uint8, or NULL)
 * is non-zero, and subtracted at every channel.  The fit uses the orthogonal
 * polynomials of the spectrum's own weights (no normal equations).  With
 * n_live the number of channels of non-zero fit weight: a spectrum with
 * n_live == 0 is left unchanged; one with 1 <= n_live <= degree is left
 * unchanged and its index row * npol + pol is appended (in no particular
 * order) to rank_list[rank_capacity] (device int32); *rank_count (device
 * int32) receives their number, which may exceed rank_capacity.
 */
int sdp_hip_vis_remove_continuum(int64_t nrows, int nchan, int npol, void *vis,
                                 int vis_dtype, const double *weight,
                                 const void *flags, int flag_bytes,
                                 const double *x, const uint8_t *mask,
                                 int degree, int32_t *rank_list,
                                 int rank_capacity, int32_t *rank_count,
                                 void *stream, char *errbuf,
                                 size_t errbuf_len);

/*
 * Sky-component image operations (reference src/ska_sdp_func_python/
 * sky_component/operations.py).  The image is [nplanes = nchan * npol, ny, nx]
 * in C order on the device, f32 or f64 (image_dtype), updated in place; every
 * other array is f64 / integer on the device.  Components are given in pixel
 * coordinates (origin 0, x = column, y = row).
 *
 * insert and restore are gathers over image tiles of SDP_HIP_SKYCOMP_TILE_Y
 * rows by SDP_HIP_SKYCOMP_TILE_X columns, numbered row-major (tiles_x =
 * ceil(nx / TILE_X)).  The caller lists each tile's components in CSR form:
 * tile_comp[tile_ptr[t] .. tile_ptr[t + 1]) are the indices of the components
 * that tile t must add, in ascending order.  A pixel adds its terms in that
 * order, each add rounded to the image type, so with the full list the result
 * is that of numpy's sequential `+=` bit for bit (insert) whatever the number
 * of components on a pixel.  A component missing from a tile's list is not
 * added there; an index outside [0, ncomp) is ignored.  ncomp == 0 leaves the
 * image untouched (the lists are then not read).
 *
 * sdp_hip_skycomp_insert: insert_skycomponent (:583-668) with insert_array
 * (util/array_functions.py:134-178).  Component c owns the window of `window`
 * rows and columns whose first pixel is origin[c] = (x0, y0) and adds
 *   flux[c][plane] * ((taps_y[c][i] * taps_x[c][j]) / insertsum[c])
 * to pixel (y0 + i, x0 + j); window pixels off the image are skipped.
 * "Nearest" is window 1 with tap 1 and insertsum 1.
 *
 * sdp_hip_skycomp_restore: restore_skycomponent (:671-741).  Component c at
 * xy[c] = (x, y) adds flux[c][plane] * exp(-(a dx^2 + b dx dy + c dy^2)),
 * dx = column - x, dy = row - y, to every pixel of the tiles that list it.
 * The caller may leave a component out of a tile's list only where the
 * exponent's argument exceeds 700 on the whole tile.
 *
 * sdp_hip_skycomp_nearest: the label image of voronoi_decomposition
 * (:744-783): labels[row][col] (int64) = argmin_c hypot(row - y[c], col -
 * x[c]), the first minimum on ties; ncomp >= 1.
 */
#define SDP_HIP_SKYCOMP_TILE_X 32
#define SDP_HIP_SKYCOMP_TILE_Y 8
int sdp_hip_skycomp_insert(int nplanes, int ny, int nx, void *image,
                           int image_dtype, int64_t ncomp, int window,
                           const int32_t *origin, const double *taps_y,
                           const double *taps_x, const double *insertsum,
                           const double *flux, const int64_t *tile_ptr,
                           const int32_t *tile_comp, void *stream,
                           char *errbuf, size_t errbuf_len);
int sdp_hip_skycomp_restore(int nplanes, int ny, int nx, void *image,
                            int image_dtype, int64_t ncomp, const double *xy,
                            const double *flux, double a, double b, double c,
                            const int64_t *tile_ptr, const int32_t *tile_comp,
                            void *stream, char *errbuf, size_t errbuf_len);
int sdp_hip_skycomp_nearest(int ny, int nx, int64_t ncomp, const double *xy,
                            int64_t *labels, void *stream, char *errbuf,
                            size_t errbuf_len);

/*
 * Frequency Taylor terms of image stacks (reference src/ska_sdp_func_python/
 * image/taylor_terms.py): a small real matrix applied across a stack of image
 * planes,
 *   out[k][i] = sum_c weights[k][c] * in[c][i],  0 <= i < npix.
 * in_planes and out_planes are HOST arrays of nin and nout DEVICE pointers,
 * one per plane of npix contiguous elements (separately allocated images and
 * slices of a cube may be mixed); the inputs are all f32 or all f64
 * (in_dtype), the outputs f64; weights is a host array [nout][nin].  The
 * library copies the three tables to device scratch; they may be freed when
 * the call returns.  No output plane may overlap an input or another output.
 *
 * Every output element starts from +0.0 and adds its terms in ascending c:
 * acc = acc + (w[k][c] * (double)in[c][i]), the product and the sum each
 * rounded once in fp64 -- numpy's `out[k] += in[c] * w`, bit for bit (a -0.0
 * input gives +0.0).  With min(nin, nout) <= SDP_HIP_MIX_PLANES_REGS every
 * input plane is read once and every output plane written once; beyond that
 * the call makes ceil(nout / REGS) passes, each over all inputs, with the
 * same result.  Planes aligned to 16
 * bytes are accessed 16 bytes per lane, any other plane element by element.
 * 1 <= nin, nout <= SDP_HIP_MIX_PLANES_MAX, 1 <= npix <= 2^40.
 *
 * nan_seen != NULL: set to 0 if no input element read and no output element
 * written was NaN, else to SDP_HIP_MIX_NAN_INPUT (an input was NaN),
 * SDP_HIP_MIX_NAN_OUTPUT (an output was: inf * 0 and inf - inf included) or
 * their sum; the call then synchronises the stream.  With NULL the call only
 * enqueues work.
 */
#define SDP_HIP_MIX_NAN_INPUT 1
#define SDP_HIP_MIX_NAN_OUTPUT 2
#define SDP_HIP_MIX_PLANES_REGS 8
#define SDP_HIP_MIX_PLANES_MAX 4096
int sdp_hip_mix_planes(int nin, int nout, int64_t npix,
                       const void *const *in_planes, int in_dtype,
                       double *const *out_planes, const double *weights,
                       int *nan_seen, void *stream, char *errbuf,
                       size_t errbuf_len);

/* ---- gather of image facets (image/gather_scatter.py) ----------------------
 * sdp_hip_gather_facets: an image [nplanes][ny][nx] from facets x facets
 * sub-images [nplanes][dy][dx], facet (fy, fx) with its first pixel at
 * (y0 + fy * sy, x0 + fx * sx) of the image (the raster of the reference's
 * image_raster_iter: sy = dy - 2 * overlap, facets in fy-major order), which
 * overlap where a step is smaller than the facet.  One pass: every facet pixel
 * is read once, every output pixel written once.
 *
 * dtype (SDP_HIP_F32 or SDP_HIP_F64) is the type T of the facets and of both
 * outputs.  facet_ptrs is a HOST table of facets^2 DEVICE pointers to the first
 * element of each facet, plane_strides and row_strides host tables of the
 * distance in elements between two planes and between two rows of each facet;
 * the x stride is 1.  A facet may be a view of a larger image.  taper_y[dy] and
 * taper_x[dx] are host fp64 arrays, or both NULL for weights of 1.  The library
 * copies the tables to device scratch; they may be freed when the call returns.
 * out and sumwt are contiguous device arrays [nplanes][ny][nx] that overlap no
 * facet; either may be NULL, and with out == NULL no facet is read and the three
 * facet tables may be NULL.  The call only enqueues work on `stream`.
 *
 * Per output element, over the facets that cover it in ascending fy, then
 * ascending fx, each operation rounded once in T (no fused multiply-add):
 *   acc = +0, sum = +0
 *   wt  = (T)(taper_y[j] * taper_x[i])      the product in fp64
 *   acc = acc + wt * v;  sum = sum + wt     (no tapers: acc = acc + v, wt = 1)
 *   normalise != 0:  out = sum > 0 ? acc / sum : 0;  sumwt = sum
 *   normalise == 0:  out = acc;                       sumwt = 1
 * which is the reference's image_gather_facets with overlap > 0 and with
 * overlap == 0, bit for bit (a -0.0 input gives +0.0; an uncovered pixel
 * gives +0).
 *
 * 1 <= facets <= SDP_HIP_GATHER_FACETS_MAX per axis; 1 <= dy <= ny and
 * 1 <= dx <= nx, at most 2^30 per side and 2^40 elements in all; sy, sx >= 1;
 * y0, x0 >= 0 and the last facet ends inside the image; strides >= 0.
 */
#define SDP_HIP_GATHER_FACETS_MAX 256
int sdp_hip_gather_facets(int dtype, int facets, int nplanes, int ny, int nx,
                          int dy, int dx, int y0, int x0, int sy, int sx,
                          const void *const *facet_ptrs,
                          const int64_t *plane_strides,
                          const int64_t *row_strides, const double *taper_y,
                          const double *taper_x, int normalise, void *out,
                          void *sumwt, void *stream, char *errbuf,
                          size_t errbuf_len);

/* ---- image segmentation (find_skycomponents) ---------------------------------
 * The device half of find_skycomponents (reference src/ska_sdp_func_python/
 * sky_component/operations.py:256-363, through photutils 1.8.0 detect_sources
 * and SourceCatalog and astropy 5.2.2 convolve).  `planes` are nchan (nplanes)
 * device planes [ny][nx], f32 or f64 (dtype), plane c at planes + c *
 * plane_stride elements (Stokes I of a cube [nchan][npol][ny][nx]: stride npol
 * * ny * nx); ny * nx < 2^31.  Every other array is a contiguous device array
 * [ny][nx] of int32 unless said otherwise.  The calls only enqueue work.
 *
 * sdp_hip_segment_label: per pixel
 *   mean   = (plane_0 + plane_1 + ... in channel order) / nchan, in the planes'
 *            type (numpy.sum(axis=0) / float(nchan));
 *   smooth = (sum over the ksize x ksize window centred on the pixel, rows then
 *            columns, of mean * taps[dy][dx], fp64, a product and an add each
 *            rounded once, pixels off the image 0) / tap_sum;
 *   mask   = smooth > threshold
 * and the 8-connected components of the mask.  taps is a HOST array [ksize]
 * [ksize], ksize odd and at most SDP_HIP_SEGMENT_KERNEL_MAX; ksize 1 with tap
 * 1 and tap_sum 1 is the identity.  labels[p] receives the flat index y * nx +
 * x of the first pixel, in raster order, of the component of pixel p, or -1
 * off the mask; count[r] of such a first pixel r its component's number of
 * pixels (count elsewhere is not meaningful).  *nonfinite (device int32, to
 * be zeroed by the caller) is set to 1 if a mean was not finite.  The result
 * depends on the input alone, not on the schedule.
 *
 * sdp_hip_segment_roots: keep[p] = 1 where p is the first pixel of a component
 * of at least npixels pixels, else 0.
 *
 * sdp_hip_segment_relabel: with rank the inclusive prefix sum of keep, the
 * segment map: segmap[p] = rank[labels[p]] where keep[labels[p]], else 0 --
 * the kept components numbered 1..n by their first pixel, which is the order
 * of scipy.ndimage.label.  segmap may be labels.
 *
 * sdp_hip_segment_peaks: per plane c and segment s in 1..nseg the maximum of
 * the plane over the pixels with segmap == s, values[c][s - 1] (f64; -0.0
 * counts and is returned as +0.0), and the smallest flat index of a pixel
 * that has it, indices[c][s - 1] (int64) -- photutils' max_value and
 * maxval_index.  Integer atomics only: exact and repeatable.  A segment
 * without a pixel gets 0 and -1.  The planes must be free of NaN.
 */
#define SDP_HIP_SEGMENT_TILE 32
#define SDP_HIP_SEGMENT_KERNEL_MAX 15
int sdp_hip_segment_label(int nchan, int ny, int nx, const void *planes,
                          int dtype, int64_t plane_stride, int ksize,
                          const double *taps, double tap_sum, double threshold,
                          int32_t *labels, int32_t *count, int32_t *nonfinite,
                          void *stream, char *errbuf, size_t errbuf_len);
int sdp_hip_segment_roots(int ny, int nx, const int32_t *labels,
                          const int32_t *count, int npixels, int32_t *keep,
                          void *stream, char *errbuf, size_t errbuf_len);
int sdp_hip_segment_relabel(int ny, int nx, const int32_t *labels,
                            const int32_t *keep, const int32_t *rank,
                            int32_t *segmap, void *stream, char *errbuf,
                            size_t errbuf_len);
int sdp_hip_segment_peaks(int nplanes, int ny, int nx, const void *planes,
                          int dtype, int64_t plane_stride,
                          const int32_t *segmap, int nseg, double *values,
                          int64_t *indices, void *stream, char *errbuf,
                          size_t errbuf_len);

/* ---- batched 2-D Gaussian fits (fit_skycomponent) -------------------------------
 * sdp_hip_gauss_fit: nfit independent least-squares fits of a rotated
 * Gaussian to windows of SDP_HIP_GAUSS_FIT_WINDOW x SDP_HIP_GAUSS_FIT_WINDOW
 * pixels (reference src/ska_sdp_func_python/sky_component/operations.py:
 * 835-916, astropy's LevMarLSQFitter on a Gaussian2D).
 *
 * planes, row_strides, x0 and y0 are HOST tables of length nfit.  planes[f]
 * is a DEVICE pointer to pixel (0, 0) of the plane that fit f reads, of type
 * dtype (SDP_HIP_F32 or SDP_HIP_F64, one for the call); row_strides[f] its
 * row stride in elements; the x stride is 1.  The window's first pixel is
 * (row y0[f], column x0[f]); the caller guarantees that the window lies on the
 * plane.  Different fits may read different planes, views of a cube or images
 * of their own, of different sizes.  The library copies the tables to device
 * scratch; they may be freed when the call returns.  The planes are only read.
 * The call only enqueues work on `stream`.
 *
 * params is a device array [nfit][6]: amplitude, x_mean, y_mean, x_stddev,
 * y_stddev, theta, the means in the plane's pixel coordinates, of
 *   g = A exp(-(a dx^2 + b dx dy + c dy^2))
 *   a = (cos^2 t / sx^2 + sin^2 t / sy^2) / 2
 *   b = (sin 2t / sx^2 - sin 2t / sy^2) / 2
 *   c = (sin^2 t / sx^2 + cos^2 t / sy^2) / 2
 * minimising the unweighted sum over the window of (g - z)^2, in fp64 whatever
 * the pixel type, both standard deviations bounded below by FLT_MIN.  The
 * start is A = max z, the means at the window's centre pixel, sx = sy = 1,
 * t = 0.  The solver is Levenberg-Marquardt in More's trust-region form (the
 * algorithm of MINPACK's lmder) on the normal equations, run until the trust
 * radius falls below 1e-12 |D x| or the cost no longer decreases in fp64; at
 * most max_iter (>= 1) model evaluations.
 *
 * status (device int32 [nfit]): 0 converged, 1 max_iter reached (params hold
 * the last accepted iterate), 2 a window pixel or an iterate was not finite
 * (params are NaN).  niter (device int32 [nfit], or NULL) receives the number
 * of model evaluations.  A fit's result depends on its window and its
 * position alone: not on nfit, nor on what else the call fits.
 */
#define SDP_HIP_GAUSS_FIT_WINDOW 15
int sdp_hip_gauss_fit(int nfit, const void *const *planes, int dtype,
                      const int64_t *row_strides, const int32_t *x0,
                      const int32_t *y0, int max_iter, double *params,
                      int32_t *status, int32_t *niter, void *stream,
                      char *errbuf, size_t errbuf_len);

/* ---- bandpass resampling (calibration/beamformer_utils.py) -----------------
 * The gain spectra of a table re-channelised (reference src/
 * ska_sdp_func_python/calibration/beamformer_utils.py:273-491).  gain is a
 * device array [nrows][c_in][nrec][nrec] complex128, a row one (time,
 * antenna) pair, out a device array [nrows][c_out][nrec][nrec] complex128,
 * both contiguous and aligned to 16 bytes, nrec 1 or 2.  All tables are
 * DEVICE arrays; the calls only enqueue work on `stream`, so the tables stay
 * allocated until it has run.  A row's result depends on that row alone: the
 * same bits alone, in any batch and on any run.  fp64, no contraction.
 *
 * sdp_hip_resample_polyfit: the unweighted least-squares polynomial of
 * `degree` (0 .. SDP_HIP_BANDPASS_MAX_DEGREE) through the input channels
 * edges[s] .. edges[s + 1] - 1 of each of nseg segments (1 ..
 * SDP_HIP_BANDPASS_MAX_SEGMENTS; int32 edges[nseg + 1], ascending within
 * 0 .. c_in), evaluated at the output channels.  The caller supplies the fit
 * factored through polynomials p_0 .. p_degree that are orthonormal under the
 * unit-weight inner product on their segment's input channels:
 *   q[d][c]   (double [degree + 1][c_in])  p_d of the segment of c, at c
 *   e[co][d]  (double [c_out][degree + 1]) p_d of segment seg[co], at co
 *   seg[co]   (int32 [c_out]) the segment of output channel co, or -1
 *   out[co] = sum_d e[co][d] * (sum_{c in seg[co]} q[d][c] * gain[c])
 * per real and imaginary part of every matrix element.  An output channel
 * with seg -1 (or a value outside 0 .. nseg - 1) is written NaN + NaN j.
 * c_in >= 2.  The inner sums are formed by 256 lanes striding over the
 * segment's channels, an xor butterfly over each wavefront's 64 lanes and
 * the four wavefronts' values added in ascending order; the outer sum starts
 * from e[co][0] * coef[0] and adds ascending d.
 *
 * sdp_hip_resample_interp: numpy.interp on complex data, bit for bit.
 * x_in [c_in] and x_out [c_out] are the abscissae (double), interval [c_out]
 * (int32) what the host's search gives for each x_out:
 *   -2            x_out is NaN: the result is x_out + 0 j
 *   -1            below x_in[0]: gain[0]
 *   0 .. c_in-2   x_in[j] <= x_out < x_in[j + 1]: gain[j] if x_out == x_in[j],
 *                 else per component slope = (y[j+1] - y[j]) * (1 / (x_in[j+1]
 *                 - x_in[j])) and slope * (x_out - x_in[j]) + y[j]; if that is
 *                 NaN, slope * (x_out - x_in[j+1]) + y[j+1]; if that is NaN
 *                 too and y[j] == y[j+1], y[j]
 *   >= c_in-1     at or above the last knot: gain[c_in - 1]
 */
#define SDP_HIP_BANDPASS_MAX_DEGREE 7
#define SDP_HIP_BANDPASS_MAX_SEGMENTS 64
int sdp_hip_resample_polyfit(int64_t nrows, int c_in, int c_out, int nrec,
                             int degree, int nseg, const void *gain, void *out,
                             const double *q, const double *e,
                             const int32_t *seg, const int32_t *edges,
                             void *stream, char *errbuf, size_t errbuf_len);
int sdp_hip_resample_interp(int64_t nrows, int c_in, int c_out, int nrec,
                            const void *gain, void *out, const double *x_in,
                            const double *x_out, const int32_t *interval,
                            void *stream, char *errbuf, size_t errbuf_len);

/* ---- sums of imaging results and clean thresholds (imaging/imaging_helpers.py)
 * sdp_hip_sum_planes: one output cube from ncube input cubes of nplane planes
 * with npix pixels each (reference src/ska_sdp_func_python/imaging/
 * imaging_helpers.py:25-93).  in_cubes is a HOST array of ncube DEVICE
 * pointers; every cube is contiguous, plane p of cube n at in_cubes[n] +
 * p * npix elements; the cubes and out are all f32 or all f64 (dtype).  The
 * library copies the pointer table to device scratch.  One launch for all
 * planes; every input is read once and the output written once.  The call
 * only enqueues work on `stream`.
 *
 * weights != NULL (weighted mode): weights [ncube][nplane] and sumwt [nplane]
 * are DEVICE arrays of doubles that stay allocated until the stream has run.
 * Every element starts from +0.0 and adds weights[n][p] * (double)in[n][p][i]
 * in ascending n, the product and the sum each rounded once in fp64.  With
 * normalise != 0 the element becomes acc / sumwt[p] (a division) where
 * sumwt[p] > 0 and +0.0 elsewhere, whatever acc is; sumwt may be NULL with
 * normalise == 0.  An f32 output is rounded once on the store.  For f64 this
 * is numpy's `im += w[..., None, None] * pixels` over the list followed by
 * normalise_sumwt, bit for bit.  out overlaps no input.
 *
 * weights == NULL (plain mode): acc = in[0], then acc = acc + in[n] for n =
 * 1 .. ncube - 1 in the element type -- numpy's `a += b`, and exact for
 * complex data passed as its real view.  out overlaps no input, except that
 * it may be in_cubes[0] itself.
 *
 * 1 <= ncube <= SDP_HIP_SUM_PLANES_MAX, nplane * npix <= 2^40.
 *
 * sdp_hip_peak_abs: the largest magnitude in one cube [nchan][npol][ny][nx],
 * f32 or f64 (dtype), with x contiguous and the distances between rows,
 * polarisations and channels given in elements (>= 0), so that a sub-image
 * that is a view of a larger image needs no copy (reference :96-150).
 *   SDP_HIP_PEAK_MOMENT0  max over pol, y, x of |(sum_c (double)x[c]) / nchan|,
 *                         the sum from +0.0 in ascending c in fp64, divided
 *                         by (double)nchan
 *   SDP_HIP_PEAK_REFCHAN  max over pol, y, x of |x[nchan / 2]|
 * *peak (HOST) receives the maximum over the values that are not NaN (0 if
 * there is none), *nan_seen (HOST) 0 or the sum of SDP_HIP_PEAK_NAN_INPUT (an
 * element read was NaN) and SDP_HIP_PEAK_NAN_MEAN (a channel mean was: inf -
 * inf included).  The maximum is taken with integer atomics on the bit
 * pattern of the non-negative doubles: the same on every run.  The call waits
 * for the stream.  npol * ny * ceil(nx / (16 / sizeof(T))) < 2^31.
 */
#define SDP_HIP_SUM_PLANES_MAX 4096
#define SDP_HIP_PEAK_MOMENT0 0
#define SDP_HIP_PEAK_REFCHAN 1
#define SDP_HIP_PEAK_NAN_INPUT 1
#define SDP_HIP_PEAK_NAN_MEAN 2
int sdp_hip_sum_planes(int ncube, int64_t nplane, int64_t npix,
                       const void *const *in_cubes, int dtype, void *out,
                       const double *weights, const double *sumwt,
                       int normalise, void *stream, char *errbuf,
                       size_t errbuf_len);
int sdp_hip_peak_abs(int mode, int nchan, int npol, int ny, int nx,
                     const void *cube, int dtype, int64_t chan_stride,
                     int64_t pol_stride, int64_t row_stride, double *peak,
                     int *nan_seen, void *stream, char *errbuf,
                     size_t errbuf_len);

/* ---- oversampled w-projection kernels (grid_data/convolution_functions.py)
 * sdp_hip_wkernel_create: the convolution functions of nw w planes, sampled
 * from the centred inverse FFT of a far field of npixel x npixel pixels padded
 * to npad = oversampling * npixel, without ever forming the padded plane.
 * With os = oversampling, h = os / 2, nd = 2 h + 1 and c = npixel / 2, plane
 * (b, z) of the result is
 *   cf[b][z][iv][iu][kv][ku] = (1 / npixel^2) sum_y sum_x
 *        e(jv, y) * a[b][z][y][x] * e(ju, x)
 *   jv = os * (kv - support / 2) - (iv - h),  ju likewise from ku and iu
 *   e(j, x) = exp(+2 pi i ((j * (x - c)) mod npad) / npad)
 * which is os * os times element [npad / 2 + jv][npad / 2 + ju] of that
 * inverse FFT.  The far field is
 *   a[b][z][y][x] = beam(w[z], y, x) * (taper[y] * taper[x]) * pb[b][y][x]
 *   r2 = fov * fov * (((y - c) / npixel)^2 + ((x - c) / npixel)^2)
 *   beam = exp(i * ((-2 pi) * -w[z]) * (1 - sqrt(1 - r2))),
 *          0 where r2 >= 1, 1 where r2 == 0
 * in fp64 with every operation rounded once (the expression of the
 * reference's w_beam for -w[z], cancellation in 1 - sqrt(1 - r2) included).
 * taper == NULL and pb == NULL stand for ones; with pb == NULL npb is 1.
 *
 * w [nw] and taper [npixel] are DEVICE doubles, pb [npb][npixel][npixel] and
 * cf [npb][nw][nd][nd][support][support] DEVICE complex128, all contiguous.
 * The exponent of e() is reduced as an integer before sincospi, so every
 * twiddle is accurate to an ulp whatever npad is.  The sums run as two complex
 * matrix products per plane in plain fp64 FMAs, x first, each sum in
 * ascending index from +0: no atomics, and the bits of a plane depend on
 * nothing but w[z], pb[b] and the geometry -- not on nw, on the other planes
 * of the call or on how the library chunks them.  Samples with equal (jv, ju)
 * have equal bits: for an even os, [iu = 2 h][ku] equals [iu = 0][ku - 1].
 * The call only enqueues work on `stream`; scratch is the library's.
 *
 * npixel even, support + 2 <= npixel <= 4096; support even, >= 2; os >= 1;
 * nd * support <= 32768; nw, npb >= 1; npb * nw < 2^31.
 */
int sdp_hip_wkernel_create(int npixel, int oversampling, int support, int nw,
                           int npb, double field_of_view, const double *w,
                           const double *taper, const void *pb, void *cf,
                           void *stream, char *errbuf, size_t errbuf_len);

#ifdef __cplusplus
}
#endif
#endif /* SKA_SDP_HIP_H */
