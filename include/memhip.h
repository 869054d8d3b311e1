/*
 * memhip.h -- C ABI of libmemhip.so: the MI355X (gfx950) kernels behind the
 * MEM (tum-vision/mem) pretraining hot path.
 *
 * The reference has no FFI of its own (it is pure Python):
 * the drop-in boundary is its Python surface, mirrored in the mem_amd package, and
 * THIS header is what that mirror binds with ctypes.  Each entry point cites
 * the reference code it replaces (paths relative to /root/reference).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes only; pointers are caller-owned DEVICE buffers
 *     (tensor.data_ptr()) unless a parameter is documented "host".
 *   - no allocation, no host synchronisation, no global mutable state inside
 *     that the product path writes; scratch comes in through (workspace,
 *     workspace_bytes); work is enqueued on `stream` (a hipStream_t passed as
 *     void*; NULL = default stream).  The two exceptions, both explicit calls:
 *     memhip_set_option (a process-wide kernel-selection table for A/B
 *     measurements; the mem_amd package never calls it outside tools and
 *     tests) and memhip_stream_reserve_cus (a reservation keyed by the
 *     caller's stream handle, set and cleared by the data-parallel reducer).
 *   - return 0 on success, a negative MEMHIP_E* code on failure; a message is
 *     available from memhip_last_error() (thread-local).  No C++ exception
 *     crosses the boundary.
 *   - "rows_pad": token-major activation matrices are allocated with their row
 *     count rounded up to a multiple of 128 and zero-filled once; kernels never
 *     write rows >= rows.
 */
#ifndef MEMHIP_H
#define MEMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEMHIP_ABI_VERSION 10  /* 10: the rasterizer takes one args struct: memhip_rasterize and memhip_rasterize_plan read the same memhip_raster_args_t; the
                                  memhip_rasterize_f64 / _aug_f64 / _var_f64 / _binned_f64 / _workspace / _binned_workspace symbols are gone (additive since: memhip_convt2d_nhwc, memhip_convt_plan, memhip_kl_uniform_rows of the tokenizer's decoder; memhip_conv_wgrad_nhwc / _plan / _workspace with memhip_conv_wgrad_args_t, memhip_relu_bwd_colsum / _workspace of dVAE training; memhip_seg_axis_table / _seg_plan / _seg_ce / _seg_confusion with memhip_seg_args_t of the segmentation loss; memhip_segdata_resize_hist / _norm / _geom with memhip_segdata_args_t of the segmentation data chain; memhip_seg_ohem_keys / _seg_ohem_select / _seg_ce_w / _seg_ohem_plan with memhip_segohem_args_t of class weights and OHEM in the segmentation loss); 9: the tokenizer takes one args struct: memhip_conv2d_nhwc and memhip_conv_plan read the same memhip_conv_args_t; one
                                  memhip_nchw_to_padded_nhwc4 and one memhip_argmax_rows with a mode argument; the per-mode symbols (_bf16 / _f32 / _f32_dyn / _f32_ex / _f16x2) are gone;
                                  8: one entry point per backward family, optional features as struct fields (memhip_branch_bwd, memhip_layernorm_bwd_branch,
                                  memhip_attn_bwd take an args struct; memhip_gemm_bf16_tn takes the workspace; the *_map / *_drop / *_out / *_ws symbols are gone; additive since: the memhip_neck_* entry points of the feature-pyramid necks);
                                  7: the finetuning recipe (memhip_mixup, memhip_mix_targets, memhip_ce_soft, memhip_ema_update), and -- additive, no
                                  existing signature changed, so the number stays -- memhip_pool_tokens / memhip_pool_tokens_bwd, memhip_gemm_bf16_nt_plan, memhip_tokens_to_maps / memhip_maps_to_tokens_add, memhip_conv_plan, memhip_gemm_bf16_tn_plan / memhip_gemm_bf16_tn_plan_workspace; 6: element-wise dropout (memhip_dropout_t, epilogue RESIDUAL_DROP, memhip_gemm_args_t.dropout, the
                                  dropout in the row kernels); 5 (round 6): memhip_build_flags, the attention backward's workspace, memhip_attn_bwd_workspace; 4 (round 5): epilogues 6 / 7 carry the stored GELU derivative as FP16 (since round 4), certified-tokenizer entry points */

#define MEMHIP_OK 0
#define MEMHIP_EINVAL (-1)   /* bad argument (shape / alignment / null) */
#define MEMHIP_EWORKSPACE (-2) /* workspace too small */
#define MEMHIP_ELAUNCH (-3)  /* hip launch / runtime error */
#define MEMHIP_EUNSUPPORTED (-4)

typedef void* memhip_stream_t;

int memhip_abi_version(void);
const char* memhip_last_error(void);
/* Name of the device code object this library was built for ("gfx950"). */
const char* memhip_arch(void);
/* Extra compiler flags this library was built with ("" for the shipped build; a measurement build made by
 * tools/build_variant.sh names its -D switches here, and bench.py prints them next to the path of the library it measured). */
const char* memhip_build_flags(void);
/* Kernel-selection switches for A/B measurements (tools/): the library reads NO environment variable; the only
 * process-wide state is this explicit table.  Names: "gemm_p8", "gemm256", "gemm_split", "gemm_p8_half", "tn_p8",
 * "raster_lds", "attn16" (0/1, default 1 = shipped dispatch), "gemm_p8_min_n" (768), "gemm256_min_n" (1024),
 * "attn16_stagger" (40000) / "attn16_stagger_fwd" (0): cycles by which the 14x14 attention workgroups with the smaller share
 * of samples start late at most, "gemm_stagger" (0): the same for the persistent GEMM workgroups, cycles per K-tile;
 * round 5: "attn_win" (1: windows 40 / 20 tokens wide and longer than 256 tokens run on the slot-layout kernels of
 * attn_win.hip, 0: attn_stream.hip), "gemm_p8_pair" (1: the full rounds and the ragged round of an NT product are ONE
 * launch, 0: two launches), "tn_group" (1: memhip_gemm_bf16_tn_group runs its products as one grid, 0: one by one);
 * round 6: "conv_waves" (16: the fp16x2 tokenizer convolutions run 8 waves per workgroup and the phase-interleaved 256 x 128 tile
 * on every layer whose grid fills the chip twice; 32: that tile at every size; 8: 8 waves, 128 x 128 tiles only; 4: 4 waves, one per SIMD),
 * "raster_bands" (0: the binned rasterizer chooses the bands per sample from the batch size; n > 0: n bands, raised to
 * the fewest the canvas allows).
 * Unknown name: MEMHIP_EINVAL.  Results do not depend on any option (same contract, different kernel or timing). */
int memhip_set_option(const char* name, int value);
int memhip_get_option(const char* name, int* value);
/* CUs that launches on `stream` leave free (rounded up to a multiple of 8: every XCD gives up the same number; 0 clears
 * it).  The persistent one-workgroup-per-CU launches (GEMMs, weight gradients, attention) size their grids for the device's
 * CUs minus this: the data-parallel reducer sets it on ITS engine's streams while gradient buckets are in flight, so that
 * RCCL's channel kernels find CUs of their own (mem_amd/parallel.py; DDP: mem/run_mem_pretraining.py:365-367).  Scoped to
 * the caller's stream handle -- another engine / stream of the process is not affected; at most 32 streams at a time. */
int memhip_stream_reserve_cus(memhip_stream_t stream, int cus);

/* ------------------------------------------------------------------------
 * Event stream -> voxel/histogram image
 * replaces EventArrToImg.__call__            mem/datasets.py:566-595
 * ------------------------------------------------------------------------
 * ev        f64 [n_total, 4] rows [x, y, t, p] (the reference's (N,4) float64
 *           layout, mem/dataset_folder.py:275-302), samples concatenated
 * offsets   i64 [B+1] CSR row offsets of each sample inside ev
 * out       u8  [B, 3, H, W] planar [pos, tss, neg] (the reference returns the
 *           same bytes viewed as (H, W, 3); the Python mirror transposes)
 * status    i32 [B]  out: number of events of sample b whose flat pixel index
 *           x + W*y fell outside [-H*W, H*W) (the reference raises IndexError)
 * workspace device scratch of memhip_raster_plan_t.ws_bytes bytes
 * Semantics: x,y truncated toward zero; only p == +1 / p == -1 count; counts
 * are exact mod 256; NumPy negative-index wrap kept; time surface (optional)
 * = (t - tmin) / (tmax - tmin) * 255 truncated to u8, last event in array
 * order wins.  The call is memhip_rasterize (memhip_raster_args_t), below the
 * augmentation record it carries.
 */

/* Event-level augmentations fused into the rasterizer's single read of the
 * events (no intermediate (N',4) arrays):
 * replaces ReshapeScaleXandY  mem/datasets.py:464-485   x*=scale_x, y*=scale_y
 *          RandomTimeFlip     mem/datasets.py:598-609   reverse order, t<-t_last-t, p<- -p
 *          Aug_FlipEvsAlongX  mem/datasets.py:501-521   x <- flip_w-1-x
 *          Aug_RandomShiftEvs mem/datasets.py:524-549   x+=shift_x, y+=shift_y, keep
 *                                                       0<=x<filt_w and 0<=y<filt_h
 * applied per event in exactly that order, in float64 like the reference.
 * (SliceRandomMaxEvs, datasets.py:488-498, is a contiguous window: express it
 * through `offsets`.)  The random draws stay with the caller (host), so parity
 * is draw for draw.  aug = device array of B records, or NULL for none.
 */
typedef struct memhip_event_aug {
  double scale_x, scale_y;   /* 1.0 = off */
  int32_t time_flip;         /* 0/1 */
  int32_t flip_x;            /* 0/1 */
  int64_t flip_w;            /* W used by the x flip */
  int32_t shift_x, shift_y;
  int32_t do_filter;         /* 0/1: apply the bounds filter of Aug_RandomShiftEvs */
  int32_t filt_w, filt_h;
  int32_t infer;             /* MEMHIP_AUG_INFER_* bits: fields that memhip_aug_resolve fills from the data (0 = none) */
} memhip_event_aug_t;
#define MEMHIP_AUG_INFER_FLIP_W 1
#define MEMHIP_AUG_INFER_FILT_W 2
#define MEMHIP_AUG_INFER_FILT_H 4

/* The one rasterizer call (ABI 10): a host struct, read at the call.  Four kernel families compute the same image:
 *   MEMHIP_RASTER_BINNED      two streaming passes (events -> 2-byte pixel keys sorted by band of the canvas -> LDS counters per
 *                             band) instead of one global atomic per event: long streams (N-ImageNet scale, BASELINE
 *                             configs[3]) and, measured, every smaller batch too.  No time surface; H*W <= 64 * 40000 pixels.
 *                             A sample whose events would exceed n_events gets status |= 1 << 30 and a zero image; status is
 *                             written for every sample by the second pass.
 *   MEMHIP_RASTER_LDS         one pass, counters privatised in LDS per band of rows: small canvases without time surface.
 *   MEMHIP_RASTER_GLOBAL      one global u32 atomic per event and a folding pass: any canvas, the time surface.
 *   MEMHIP_RASTER_GLOBAL_VAR  the same with per-sample canvases (`dims`, written by memhip_aug_resolve stage 1).
 * `form` says which may run: MEMHIP_RASTER_AUTO = binned where it applies (no time surface, no dims, canvas within the band
 * limit), else as MEMHIP_RASTER_SINGLE = LDS where it applies ("raster_lds" option on, no time surface, no dims, at most 6
 * bands of rows, `out` 4-byte aligned), else global; MEMHIP_RASTER_BINNED forces the two passes (MEMHIP_EINVAL with
 * time_surface or dims, MEMHIP_EUNSUPPORTED beyond the band limit).  B == 0 is MEMHIP_OK, nothing is read. */
enum { MEMHIP_RASTER_AUTO = 0, MEMHIP_RASTER_SINGLE = 1, MEMHIP_RASTER_BINNED = 2,        /* form (BINNED: also a family) */
       MEMHIP_RASTER_LDS = 3, MEMHIP_RASTER_GLOBAL = 4, MEMHIP_RASTER_GLOBAL_VAR = 5 };   /* family */
typedef struct memhip_raster_args {
  const double* ev;                  /* 16-byte aligned */
  const int64_t* offsets;
  const memhip_event_aug_t* aug;     /* device array of B records, or NULL for none */
  const int32_t* dims;               /* NULL: one H x W canvas for the batch.  Device i32 [B, 2]: sample b is rasterized on
                                        dims[b] = (H_b, W_b) and stored densely ([3, H_b, W_b]) at the start of its slot of 3*H*W
                                        bytes of `out` (rest of the slot zero); H, W are then the maxima */
  int32_t B, H, W, time_surface;
  int32_t form;                      /* MEMHIP_RASTER_AUTO / _SINGLE / _BINNED */
  int32_t reserved0;
  int64_t n_events;                  /* >= 0: upper bound on offsets[B] - offsets[0] (sizes the key workspace of the binned family) */
  uint8_t* out;                      /* u8 [B, 3, H, W] */
  int32_t* status;                   /* i32 [B] */
  void* workspace;                   /* device, workspace_bytes >= memhip_raster_plan_t.ws_bytes */
  size_t workspace_bytes;
} memhip_raster_args_t;
int memhip_rasterize(const memhip_raster_args_t* args, memhip_stream_t stream);

/* The dispatch of memhip_rasterize as data.  memhip_rasterize_plan takes the struct of the call and validates it like the call
 * (same messages, same return codes), except that every pointer may be NULL: only address bits are read (null and alignment; a
 * NULL pointer counts as aligned, and workspace_bytes is compared only when `workspace` is given).  It plans with the current
 * values of the "raster_lds" and "raster_bands" options for a device of device_cus CUs (< 0: the current device's); it
 * launches nothing and needs no device when device_cus is given. */
enum { MEMHIP_RASTER_K_COUNT,      /* raster_count: global atomics */
       MEMHIP_RASTER_K_FINALIZE,   /* raster_finalize: u32 bins -> u8 planes, time surface */
       MEMHIP_RASTER_K_LDS,        /* raster_lds_kernel */
       MEMHIP_RASTER_K_BIN_KEYS,   /* raster_bin_keys: pass 1 */
       MEMHIP_RASTER_K_BIN_ACCUM };/* raster_bin_accum: pass 2 */
typedef struct memhip_raster_launch {
  int32_t kernel;             /* MEMHIP_RASTER_K_* */
  int32_t grid_x, grid_y;     /* workgroups (grid_y = B) */
  int32_t block;              /* workgroup size */
  int32_t lds;                /* dynamic LDS bytes */
} memhip_raster_launch_t;
typedef struct memhip_raster_plan {
  int32_t family;             /* MEMHIP_RASTER_LDS / _GLOBAL / _GLOBAL_VAR / _BINNED; 0: B == 0, nothing to do */
  int32_t rows_per_band, bands;   /* LDS: bands of whole rows */
  int32_t band_px, nb;        /* binned: nb bands of band_px pixels (a multiple of 4), the last one shorter, none empty */
  int32_t bx;                 /* binned: the grid_x of pass 1, which pass 2 receives as an argument */
  uint64_t ws_bytes;          /* workspace the call needs */
  uint64_t off_bins, off_tstat;             /* byte offsets of the workspace's parts: single-pass forms (u32 bins, u64 tstat) */
  uint64_t off_keys, off_hdr, off_bad_slots;   /* binned (u16 keys, u32 chunk headers, i32 one slot per pass-1 workgroup) */
                              /* every part starts at a 16-byte boundary but off_bad_slots, which is 4-byte aligned: it follows
                                 the chunk headers of 129 words each directly (the layout and ws_bytes of the earlier ABIs are
                                 kept), and its int32 slots are stored and loaded one at a time */
  uint64_t clear_ws_bytes, clear_status_bytes, clear_out_bytes;   /* zeroed in front of the launches (0: not cleared) */
  int32_t count;
  memhip_raster_launch_t l[2];
} memhip_raster_plan_t;
int memhip_rasterize_plan(const memhip_raster_args_t* args, int device_cus, memhip_raster_plan_t* out);

/* Data-dependent canvases without a host round trip (mem/datasets.py:516,537-540,572-575: "W = x.max() + 1"):
 *   memhip_events_extent(raw window) -> memhip_aug_resolve(stage 0) fills the inferred flip / filter sizes of aug[b];
 *   memhip_events_extent(with aug)   -> memhip_aug_resolve(stage 1) writes the canvas dims[b] = (H_b, W_b)
 *   (fixed_h / fixed_w > 0 override; empty samples or canvases beyond hmax x wmax: dims (0,0), status |= 1 << 29);
 *   memhip_rasterize with memhip_raster_args_t.dims rasterizes sample b on its own canvas. */
int memhip_aug_resolve(const double* extent, memhip_event_aug_t* aug, int B, int stage, int fixed_h, int fixed_w,
                       int hmax, int wmax, int32_t* dims, int32_t* status, memhip_stream_t stream);

/* Per-sample extent of the (augmented) events, for the reference's data-dependent
 * canvas "W = xs.max()+1" (mem/datasets.py:516,538-540,572-575).
 * extent   f64 [B,4] out: max x, max y, min x, min y after `aug` (NULL = raw)
 *          and the bounds filter; rows of empty samples are (-inf,-inf,+inf,+inf). */
int memhip_events_extent(const double* ev, const int64_t* offsets, const memhip_event_aug_t* aug,
                         int B, double* extent, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Event record contract: raw dataset records -> the (N,4) float64 rows [x, y, t, p]
 * replaces the N-Caltech101 decode loop        process_data/process_dataset.py:48-63
 *          imgnet_npy_loader                   mem/dataset_folder.py:285-292
 *          dsec_npy_loader                     mem/dataset_folder.py:275-283
 * ------------------------------------------------------------------------
 * decode_ncaltech101: raw u8 [n_bytes] (device, 4-byte aligned) of 5-byte records: byte0 -> column 0,
 *   byte1 -> column 1, p = bit 7 of byte2 -> 2p-1, t = (byte2 & 0x7f):byte3:byte4 big-endian (23 bits);
 *   ev f64 [n_bytes/5, 4].  n_bytes % 5 != 0 -> MEMHIP_EINVAL (the reference's loop raises on the short read).
 * events_from_columns: four device column arrays of n elements with a dtype code each ->
 *   ev[i] = [x[i], y[i], t[i], int8(int8(p[i]) * 2 - 1)] as float64 (the int8 wrap-around of
 *   `data['p'].astype(np.int8) * 2 - 1` kept; p must be bool / integer).
 * events_dsec: in [n,4] row-major of `dtype` -> out f64 rows [x, y, t, 2p-1] of the rows with y < y_limit
 *   (440 in the reference), order kept; n_out i64 (device) = number of rows written; out has room for n rows. */
#define MEMHIP_DT_U8 0
#define MEMHIP_DT_I8 1
#define MEMHIP_DT_U16 2
#define MEMHIP_DT_I16 3
#define MEMHIP_DT_U32 4
#define MEMHIP_DT_I32 5
#define MEMHIP_DT_U64 6
#define MEMHIP_DT_I64 7
#define MEMHIP_DT_F32 8
#define MEMHIP_DT_F64 9
#define MEMHIP_DT_BOOL 10
int memhip_decode_ncaltech101(const uint8_t* raw, int64_t n_bytes, double* ev, memhip_stream_t stream);
int memhip_events_from_columns(const void* x, int x_dtype, const void* y, int y_dtype, const void* t, int t_dtype,
                               const void* p, int p_dtype, int64_t n, double* ev, memhip_stream_t stream);
size_t memhip_events_dsec_workspace(int64_t n);
int memhip_events_dsec(const void* in, int dtype, int64_t n, double y_limit, double* out, int64_t* n_out,
                       void* workspace, size_t workspace_bytes, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Image-space augmentation chain, batched with per-sample parameters (host draws, device arithmetic)
 * replaces ToTensor + Resize(bilinear, antialias=True) / RandomCrop(pad_if_needed)   mem/datasets.py:637-642
 *          ToUnit8 -> EventRandAugment(num_ops=2, 14 ops) -> ToFloat32               mem/datasets.py:655-658,
 *                                                                                    mem/transforms.py:292-484
 *          ColorJitter(brightness, 0, saturation)                                    mem/datasets.py:34-38
 * (torchvision tensor ops in the reference: uint8 images, float32 arithmetic, truncating casts, torch.round after
 * resampling; restated in oracle/aug_t.py.)
 * ------------------------------------------------------------------------
 * resample_to_f32: in u8 = B slots of slot_bytes, sample b stored densely as [3, h_b, w_b] (dims i32 [B,2], or
 *   fixed_h / fixed_w when dims is NULL) -> out f32 [B,3,OH,OW] = value / 255 resampled:
 *   mode 0 Resize((OH,OW), BILINEAR, antialias=True) per sample (separable triangle filter, horizontal first);
 *   mode 1 crop window (OH,OW) at offs[b] = (top, left) (NULL = 0,0) of the image zero-padded on BOTH sides by the
 *          deficit when it is smaller than the window (RandomCrop(pad_if_needed=True)).
 * to_uint8: y = (255 * x).to(uint8)  (ToUnit8, transforms.py:341-348).
 * rand_augment_u8: one op per sample on u8 [B,3,H,W] (out != in); ops = device array of B records
 *   { int32 op (index into ['Identity','ShearX','ShearY','TranslateX','TranslateY','Rotate','Brightness','Color',
 *   'Contrast','Sharpness','Posterize','Solarize','AutoContrast','Equalize']); float mag (Posterize bits / Solarize
 *   threshold); float theta[6] }: affine ops: theta = torchvision's inverse affine matrix as float32; blend ops
 *   (Brightness/Color/Contrast/Sharpness): theta[1] = float32(ratio), theta[0] = float32(1 - ratio), ratio = 1 + magnitude.
 * color_jitter: in u8 (value / 255 first = ToFloat32) or f32 [B,3,H,W] -> out f32 [B,out_chans,H,W] (2 = [pos,neg]);
 *   params = device array of B records { int32 order (0 none, 1 brightness, 2 saturation, 3 b then s, 4 s then b);
 *   float bf, 1-bf, sf, 1-sf } or NULL (conversion / channel drop only). */
int memhip_resample_to_f32(const uint8_t* in, const int32_t* dims, int64_t slot_bytes, int fixed_h, int fixed_w, int mode,
                           const int32_t* offs, int B, int OH, int OW, float* out, memhip_stream_t stream);
int memhip_to_uint8(const float* x, int64_t n, uint8_t* y, memhip_stream_t stream);
int memhip_rand_augment_u8(const uint8_t* in, uint8_t* out, const void* ops, int B, int H, int W, memhip_stream_t stream);
int memhip_color_jitter(const void* in, int in_is_u8, int B, int H, int W, const void* params, float* out, int out_chans,
                        memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Tensor-level event transforms, fused
 * replaces ToTensor (/255), RemoveTimesurface, RemoveHotPixels, LogTransform,
 * GammaTransform, NormalizeEvent            mem/transforms.py:200-275
 * in the order of build_transformNPY        mem/datasets.py:637-653
 * ------------------------------------------------------------------------
 * in        u8 [B,3,H,W] (in_is_u8=1: value/255 first) or f32 [B,3,H,W]
 * out       f32 [B, out_chans, H, W]; out_chans = 3 keeps [pos,tss,neg],
 *           out_chans = 2 keeps [pos,neg] (= x[:, 0::2], the "2-bin voxel")
 * flags     bit0 remove_timesurface, bit1 remove_hot_pixels, bit2 log,
 *           bit3 gamma, bit4 normalize
 */
#define MEMHIP_EV_RM_TS 1
#define MEMHIP_EV_HOTPIX 2
#define MEMHIP_EV_LOG 4
#define MEMHIP_EV_GAMMA 8
#define MEMHIP_EV_NORMALIZE 16
int memhip_event_norm(const void* in, int in_is_u8, int B, int H, int W, int flags,
                      float num_stds, float gamma, float* out, int out_chans,
                      memhip_stream_t stream);
/* RemoveHotPixels(num_hot_pixels = k) form of the same chain     mem/transforms.py:257-263
 * (the k largest entries of x[0::2].flatten() are hot; k is clamped to sum / 4 like the
 * reference; both polarities of a hot pixel are zeroed).  Equal values at the selection
 * boundary: the reference leaves their order to torch.argsort(stable=False); here the
 * larger flat index is taken.  hot_keys: u64 [B] scratch (the per-sample selection key).
 * MEMHIP_EV_HOTPIX is implied. */
int memhip_event_norm_topk(const void* in, int in_is_u8, int B, int H, int W, int flags,
                           int num_hot_pixels, float gamma, float* out, int out_chans,
                           uint64_t* hot_keys, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Mask generators (HOST code: bit-exact CPython `random` semantics need
 * glibc exp/log/sqrt and a sequential MT19937 stream)
 * replaces MaskingGenerator.__call__         mem/masking_generator.py:44-81
 *          MaskingGeneratorRandomLocation    mem/masking_generator.py:106-116
 * ------------------------------------------------------------------------
 * mt_state  host u32 [625]: the 624 MT19937 words + position, exactly the
 *           tuple random.getstate()[1]; updated in place.
 * out       host u8 [n_masks, H, W] (0/1)
 */
int memhip_mt_seed(uint32_t* mt_state, const uint32_t* key, int key_len);
double memhip_mt_random(uint32_t* mt_state);
int memhip_mask_blockwise(uint32_t* mt_state, int H, int W, int num_masking_patches,
                          int min_num_patches, int max_num_patches, double log_aspect_lo,
                          double log_aspect_hi, int n_masks, uint8_t* out);
int memhip_mask_random_location(uint32_t* mt_state, int H, int W, int num_masking_patches,
                                int n_masks, uint8_t* out);

/* ------------------------------------------------------------------------
 * bf16 MFMA GEMM  C[M,N] = A[M,K] * B[N,K]^T  (+ fused epilogue)
 * replaces every F.linear / nn.Linear / nn.Conv2d(k=s=patch) of the ViT:
 *   patch embed  mem/modeling_finetune.py:203,209   qkv  :132-133   proj :155
 *   fc1+GELU     :61-68    fc2 :69    lm_head  mem/modeling_pretrain.py:59,126
 * and their dgrad / wgrad products in backward.
 * ------------------------------------------------------------------------
 * A, B are bf16 row-major with the reduction dimension contiguous (lda, ldb in
 * elements, multiples of 8; K a multiple of 64).  fp32 accumulate.  Output
 * rows >= M / cols >= N are never written.
 */
#define MEMHIP_EPI_BIAS_BF16 0   /* out0 bf16 = bf16(acc+bias); cols < colscale_n then *= colscale (q*scale, :137) */
#define MEMHIP_EPI_BIAS_GELU 1   /* out0 bf16 = h = bf16(acc+bias); out1 bf16 = gelu(h)       (:66-68) */
#define MEMHIP_EPI_RESIDUAL 2    /* y=bf16(acc+bias) -> out0 (may be NULL); resid f32 = (aux f32 or resid) + drop_path(vec1*y) (:187-188) */
#define MEMHIP_EPI_DGELU 3       /* out0 bf16 = bf16(acc) * gelu'(aux bf16)                   (GELU backward) */
#define MEMHIP_EPI_F32 4         /* out0 f32 (+)= acc                                         (weight gradients) */
#define MEMHIP_EPI_PATCH_EMBED 5 /* resid f32[b*(L+1)+1+p] = bf16(acc+bias)*(1-w) + vec1*w    (modeling_pretrain.py:101-108) */
#define MEMHIP_EPI_BIAS_GELU_DG 6 /* as BIAS_GELU, but out0 = gelu'(h) as FP16 (16 bits per value like bf16, 11 significant bits:
                                    gelu' lies in [-0.13, 1.13]) instead of h: the GELU backward then is a plain product
                                    (MUL_AUX) -- erf/exp are evaluated once, in the forward epilogue */
#define MEMHIP_EPI_MUL_AUX 7     /* out0 bf16 = bf16(acc) * aux fp16  (+ colsum)               (GELU backward with stored gelu') */
#define MEMHIP_EPI_RESIDUAL_DROP 8 /* RESIDUAL with element-wise dropout of the branch (proj_drop / Mlp.drop, mem/modeling_finetune.py:
                                    70,155,185-188): y = bf16(acc + bias); z = fp32(y * keep * scale) (one fp32 rounding;
                                    keep = 0 gives +-0); then exactly RESIDUAL's arithmetic with z for y: gamma * z (own rounding),
                                    drop path (/ keep_prob, * rowmask), + residual input.  `dropout` must be non-NULL, out0 NULL.
                                    The mask row is the residual-stream row that the RESIDUAL epilogue resolves (sample_map
                                    included) + dropout->row0; see memhip_dropout_t. */

/* ------------------------------------------------------------------------
 * Element-wise dropout (nn.Dropout, p = drop_rate of the finetuning model; mem/modeling_finetune.py:64,70,125-126,155,271,343)
 * ------------------------------------------------------------------------
 * THE MASK CONTRACT.  An element is (site, row, col):
 *   row   the row of the fp32 residual stream, sample * T + token, counted with the ORIGINAL sample index (never a compact
 *         work-skipping index or a row of a split half): masks do not depend on work skipping, stream splits or b0 / b1.
 *         A call that addresses a buffer whose row 0 is residual-stream row r0 passes row0 = r0.
 *   col   in [0, D), D a multiple of 8.
 *   site  block i's attention branch 2i, its MLP branch 2i + 1, pos_drop 2 * depth.  Decode heads (Dropout2d: row = sample,
 *         col = channel) take MEMHIP_DROPOUT_SITE_HEAD = 0x48454144 + the head's number, far above 2 * depth for any depth.
 * One Philox4x32-10 call per 8 columns: key = (key0, key1), counter = (row, col / 8, site, 0).  Column 8 * (col / 8) + j takes
 * the 16-bit half (j & 1) of output word (j >> 1), low half first; the element is KEPT iff that half >= thr = round(p * 65536),
 * and a kept value is multiplied by scale = 1 / (1 - p) (torch's scale).  The keep rate is 1 - thr / 65536 (within 7.6e-6
 * of 1 - p).  0 <= p < 1; p = 0 (thr = 0) keeps everything.  The masks follow nn.Dropout's law, not torch's stream.
 * Every kernel below that takes a memhip_dropout_t and memhip_dropout_mask compute the bits with the same device function.
 * The struct is read on the HOST at the call (its values become kernel arguments); NULL = no dropout where allowed. */
typedef struct memhip_dropout {
  uint32_t key0, key1;   /* per-step key */
  uint32_t site;
  uint32_t thr;          /* round(p * 65536) */
  float scale;           /* 1 / (1 - p) */
  int32_t row0;          /* residual-stream row of row 0 of the addressed buffer */
} memhip_dropout_t;
/* out u8 [rows, cols] = keep bit (0/1) of rows row0 .. row0 + rows - 1 (the struct's row0 is added), columns 0 .. cols - 1
 * (cols % 8 == 0).  For tests and inspection; not on the training step. */
int memhip_dropout_mask(const memhip_dropout_t* d, int row0, int rows, int cols, uint8_t* out, memhip_stream_t stream);
/* x f32 [rows, D] (ld ldx) *= keep * scale in place, rows = residual-stream rows row0 .. (pos_drop after the position
 * embedding, mem/modeling_finetune.py:343; its backward applies the same mask to the gradient). */
int memhip_dropout_rows_f32(const memhip_dropout_t* d, float* x, int64_t ldx, int rows, int D, memhip_stream_t stream);

typedef struct memhip_gemm_args {
  const void* A; const void* B;
  int64_t lda, ldb;
  int32_t M, N, K, epilogue;
  void* out0; int64_t ldo0;
  void* out1; int64_t ldo1;
  const float* bias;      /* [N] fp32 or NULL */
  const float* vec1;      /* RESIDUAL: layer-scale gamma [N] (NULL = none); PATCH_EMBED: mask_token [N] */
  float* resid; int64_t ldr;   /* fp32 residual stream */
  const void* aux; int64_t ldaux; /* DGELU: pre-activation bf16 [M,N]; PATCH_EMBED: mask u8 [M];
                                     RESIDUAL: residual INPUT f32 [M,N] (NULL = resid in place) */
  const float* rowmask;   /* RESIDUAL: stochastic-depth keep mask per sample (0/1), NULL = off */
  float keep_prob;        /* RESIDUAL: 1 - drop_prob */
  float colscale; int32_t colscale_n;
  int32_t rows_per_sample;  /* RESIDUAL: tokens per sample; PATCH_EMBED: patches per sample */
  int32_t accumulate;     /* F32: 1 = out0 += acc */
  float* colsum;          /* BIAS_BF16 / DGELU: f32 [N] += column sums of the bf16 output rows < M (the
                             bias gradient of the Linear whose grad_output this GEMM produces); NULL = off */
  const int32_t* sample_map; /* RESIDUAL, stochastic depth as WORK SKIPPING (the GEMM runs on the rows of the kept samples
                             only): output row m belongs to compact sample c = m / rows_per_sample, and its residual row in
                             `resid` / `aux` is sample_map[c] * rows_per_sample + m % rows_per_sample.  The kept branch is
                             scaled by 1 / keep_prob; rowmask must be NULL.  The array must be readable for 256 entries
                             past the last compact sample.  NULL = rows map to themselves. */
  int32_t colsum_copies;  /* > 1: `colsum` holds that many accumulator copies of N floats each (copy k at colsum + k * N;
                             all zero on entry) and a workgroup adds into copy blockIdx % copies: atomics on one address
                             serialise (~0.17 us each on gfx950), and with one copy the ~400 per column of a ViT-B
                             launch sit in the in-order vector-memory queue in front of the operand stream (measured:
                             +27 us on the 3072-wide GELU' GEMM, +100 us on a 768 x 768 one).  Fold the copies with
                             memhip_colsum_fold.  0 / 1: a single accumulator (the bias gradient itself). */
  int32_t reserved0;
  const memhip_dropout_t* dropout;  /* RESIDUAL_DROP: the branch's dropout (HOST struct, read at the call); other epilogues:
                                       must be NULL (ABI 6) */
} memhip_gemm_args_t;
int memhip_gemm_bf16_nt(const memhip_gemm_args_t* args, memhip_stream_t stream);

/* The dispatch of memhip_gemm_bf16_nt as data: which kernel form takes which rows of the product (additive to ABI 7).
 * memhip_gemm_bf16_nt_plan validates `args` like the GEMM itself and plans with the current option values for a stream
 * with stream_cus usable CUs on a device of device_cus CUs; it launches nothing and needs no device (pointers are
 * checked, never read).  The launches cover rows [0, M) once, in order. */
#define MEMHIP_NT_128 0       /* 128x128 kernel, one workgroup per tile */
#define MEMHIP_NT_G256 1      /* lockstep persistent 256x256 kernel (grid sized for device_cus) */
#define MEMHIP_NT_P8_256 2    /* phase-interleaved persistent kernel, 256-row tiles (rows % 256 == 0) */
#define MEMHIP_NT_P8_128 3    /* the same on 128-row tiles */
#define MEMHIP_NT_P8_PAIR 4   /* one launch: 256-row tiles on `rows`, 128-row tiles on the `tail_rows` behind them */
typedef struct memhip_nt_launch {
  int32_t kind;
  int32_t row0, rows;
  int32_t tail_rows;          /* P8_PAIR only */
  int32_t guard;              /* P8_128 / P8_PAIR: the 128-row range is not a multiple of 128 rows */
  int32_t copy;               /* P8_*: the kernel form that stores out0 */
  int32_t grid, tail_grid;    /* workgroups: tiles (NT_128) or min(tiles, CUs); tail_grid: the 128-row part of a pair */
} memhip_nt_launch_t;
typedef struct memhip_nt_plan { int32_t count; memhip_nt_launch_t l[2]; } memhip_nt_plan_t;
int memhip_gemm_bf16_nt_plan(const memhip_gemm_args_t* args, int stream_cus, int device_cus, memhip_nt_plan_t* out);

/* Weight-gradient GEMM  out[N,K] (+)= sum_r A[r,N] * B[r,K]  (A = dY, B = X, both token-major
 * bf16 with the reduction over ROWS): the dY^T @ X that autograd computes for every Linear /
 * Conv2d weight on the path.  No transposed copies: fragments are read with the transposing LDS
 * read; split-K over the rows with fp32 atomics.  accumulate=1: add into `out` (pre-zeroed by
 * the caller); accumulate=0: overwrite.
 * workspace: caller-owned scratch of memhip_gemm_bf16_tn_workspace(R,N,K) bytes (0 = the shape has no use for one): the per-slice
 * partial tiles are then written with plain stores and summed by a reduction pass in a fixed order (run-to-run deterministic)
 * instead of fp32 atomics (64 MB of atomics per ViT-B weight gradient otherwise).  NULL / too small: the atomic form. */
size_t memhip_gemm_bf16_tn_workspace(int R, int N, int K);
int memhip_gemm_bf16_tn(const void* A, int64_t lda, const void* B, int64_t ldb, int R, int N, int K,
                        float* out, int64_t ldo, int accumulate, void* workspace, size_t workspace_bytes,
                        memhip_stream_t stream);
/* The weight gradients of up to 4 Linear layers whose operands are ready at the same time (fc2 + fc1, proj + qkv of a
 * Block: mem/modeling_finetune.py:160-189 backward) as ONE launch: the products share one grid and one common count of row
 * slices, so a small product (768 x 768: 9 tiles) runs with the 7 row slices of its neighbour instead of the 27 it plans
 * alone to fill the chip, and the group has one reduction pass.  Each product has the contract of memhip_gemm_bf16_tn
 * (fixed sum order: run-to-run deterministic; the order differs from the single call's, so the two agree to fp32 rounding,
 * not bitwise).  workspace: memhip_gemm_bf16_tn_group_workspace(problems, count) bytes (also >= what each product needs
 * alone).  Whether a group runs as one grid is decided by tn_plan (mem_amd/csrc/gemm_tn_plan.cpp; memhip_gemm_bf16_tn_plan
 * shows the decision); a group that does not is computed product by product, each exactly as memhip_gemm_bf16_tn would
 * -- same results contract. */
typedef struct memhip_tn_problem {
  const void* A; int64_t lda;       /* dY  bf16 [R, N] */
  const void* B; int64_t ldb;       /* X   bf16 [R, K] */
  float* out; int64_t ldo;          /* dW  f32  [N, K] */
  int32_t R, N, K;
  int32_t reserved0;
} memhip_tn_problem_t;
size_t memhip_gemm_bf16_tn_group_workspace(const memhip_tn_problem_t* problems, int count);
int memhip_gemm_bf16_tn_group(const memhip_tn_problem_t* problems, int count, int accumulate, void* workspace,
                              size_t workspace_bytes, memhip_stream_t stream);

/* The dispatch of memhip_gemm_bf16_tn / _tn_group as data (additive to ABI 7): the ordered launches with their row
 * slices, grids and workspace layout.  memhip_gemm_bf16_tn_plan validates `problems` like memhip_gemm_bf16_tn_group (a single
 * call is a group of one) and plans with the current option values for a stream of stream_cus usable CUs (>= 0: no device
 * is needed; < 0: what the default stream has on the current device).  Nothing is launched; of the pointers only the address
 * bits are read (null, 16-byte alignment).  Products with R == 0 appear in no launch. */
#define MEMHIP_TN_128 0        /* gemm_tn_kernel: 128x128 tiles, row slices added with atomics (one slice, overwrite: plain stores) */
#define MEMHIP_TN_P8_ATOMIC 1  /* gemm_tn_p8_kernel<false>: 256x256 tiles, row slices added with atomics */
#define MEMHIP_TN_P8_WS 2      /* gemm_tn_p8_kernel<true> + tn_reduce_kernel: slices stored to the workspace, then summed */
#define MEMHIP_TN_P8_GROUP 3   /* gemm_tn_p8_group_kernel + tn_reduce_group_kernel: several products, one grid */
typedef struct memhip_tn_part {   /* one product inside a launch */
  int32_t problem;                /* index into `problems` */
  int32_t tiles, splits, rows_per_split;   /* the product runs tiles * splits workgroups; slice s takes rows [s, s + 1) * rows_per_split */
  int32_t wg_begin, quad_begin;   /* group: first workgroup id of the product, first float4 of it in the reduction pass */
  int64_t ws_offset;              /* floats: where the product's slabs [splits][N][K] start in the workspace */
} memhip_tn_part_t;
typedef struct memhip_tn_launch {
  int32_t kind;                   /* MEMHIP_TN_* */
  int32_t count;                  /* products covered (1 unless MEMHIP_TN_P8_GROUP) */
  int32_t grid, reduce_grid;      /* workgroups of the main kernel and of the reduction pass (0: none) */
  int32_t memset_first;           /* `out` is cleared in front of the launch */
  int32_t use_atomics;            /* the main kernel adds into `out` with atomics */
  int64_t ws_bytes;               /* workspace bytes the launch uses (0: none) */
  memhip_tn_part_t p[4];
} memhip_tn_launch_t;
typedef struct memhip_tn_plan { int32_t count; int32_t reserved0; memhip_tn_launch_t l[4]; } memhip_tn_plan_t;
int memhip_gemm_bf16_tn_plan(const memhip_tn_problem_t* problems, int count, int accumulate, const void* workspace,
                             size_t workspace_bytes, int stream_cus, memhip_tn_plan_t* out_plan);
/* memhip_gemm_bf16_tn_group_workspace as it answers on a device of device_cus CUs (count == 1: memhip_gemm_bf16_tn_workspace
 * of that shape); needs no device. */
size_t memhip_gemm_bf16_tn_plan_workspace(const memhip_tn_problem_t* problems, int count, int device_cus);
/* out f32 [C] += column sums of in bf16 [R, C]  (Linear bias gradients = grad_output.sum(0)) */
int memhip_colsum_bf16(const void* in, int64_t ld, int R, int C, float* out, memhip_stream_t stream);
/* out[n] += sum_k ws[k * N + n] for the `copies` accumulator copies a GEMM with colsum_copies > 1 filled; the copies
 * are zeroed again (ready for the next GEMM).  Same reduction order every run. */
int memhip_colsum_fold(float* ws, int copies, int N, float* out, memhip_stream_t stream);

/* Dead-row elimination in the LAST block (Block.forward, mem/modeling_finetune.py:160-189; the head reads only the masked
 * tokens' rows, mem/modeling_pretrain.py:119-126): the MLP branch of the last block runs on those rows in compact form.
 * residual_rows: out[i, :] = x[rows[i], :] + drop_path(gamma * y[i, :]) with y the bf16 output of the fc2 GEMM (+ bias) for
 * compact row i -- the arithmetic of the RESIDUAL epilogue; gamma NULL = no layer scale; rowkeep f32 [R] (0/1 per compact
 * row, NULL = no stochastic depth) with keep_prob.  scatter_rows: dst[rows[i], :] = src[i, :] (fp32 rows of D values). */
int memhip_residual_rows(const float* x, int64_t ldx, const int32_t* rows, const void* y, int64_t ldy, const float* gamma,
                         const float* rowkeep, float keep_prob, int R, int D, float* out, int64_t ldo,
                         memhip_stream_t stream);
int memhip_scatter_rows_f32(const float* src, int64_t lds, const int32_t* rows, int R, int D, float* dst, int64_t ldd,
                            memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * LayerNorm (eps 1e-6) forward / backward          mem/modeling_pretrain.py:132,
 * mem/modeling_finetune.py:166,172,184-188; final norm mem/modeling_pretrain.py:117
 * ------------------------------------------------------------------------
 * x fp32 [*, D] (residual stream), y bf16 [R, D] (what the next Linear consumes
 * under autocast), mean/rstd fp32 [R].  row_idx (i32 [R], may be NULL) selects
 * the input row of output row r: the final norm + `x[:,1:][bool_masked_pos]`
 * (modeling_pretrain.py:121-126) is one gathered LayerNorm over the masked rows.
 * backward: dres[row] (+)= dx, dgamma/dbeta fp32 [D] are ACCUMULATED.
 */
int memhip_layernorm_fwd(const float* x, int64_t ldx, const int32_t* row_idx, int R, int D,
                         const float* gamma, const float* beta, float eps, void* y_bf16, int64_t ldy,
                         float* mean, float* rstd, memhip_stream_t stream);
int memhip_layernorm_bwd(const void* dy_bf16, int64_t lddy, const float* x, int64_t ldx,
                         const int32_t* row_idx, int R, int D, const float* gamma, const float* mean,
                         const float* rstd, float* dres, int64_t lddres, int accumulate, float* dgamma,
                         float* dbeta, memhip_stream_t stream);

/* Layer-scale gradient from the weight gradient of the Linear that produced the branch:
 *   dgamma[c] = (sum_k W[c,k] * dW[c,k] + bias[c] * dbias[c]) / gamma[c]      (0 where gamma[c] == 0)
 * (x += gamma * y with y = A W^T + b: sum_m dt*y = sum_m dY*y / gamma and dW = dY^T A, dbias = colsum dY), so the
 * identity also holds with dropout of the branch: with z = keep * scale * y, dgamma = sum_m dt*z and dY = dt*gamma*keep*scale,
 * so sum_m dY*y = gamma * sum_m dt*z on both sides alike.  The
 * forward does not store y and memhip_branch_bwd / memhip_layernorm_bwd_branch run with y = NULL, dgamma = NULL.
 * W bf16 [N, ldw] (the operand the forward used), dW / dbias f32 = the gradients accumulated so far;
 * dgamma is OVERWRITTEN (it is a function of the accumulated dW). */
int memhip_layerscale_grad(const void* W_bf16, int64_t ldw, const float* dW, int64_t lddw, const float* bias,
                           const float* dbias, const float* gamma, int N, int K, float* dgamma,
                           memhip_stream_t stream);

/* Backward of `x = x + drop_path(gamma * y)` (mem/modeling_finetune.py:187-188), the residual branch whose OUTPUT gradient is
 * produced: dy = bf16(dt * gamma), dgamma += sum_m dt*y, dbias += sum_m dy with dt = dx * rowmask[m / rows_per_sample] / keep_prob.
 * Host structs, read at the call; an optional feature is a field whose NULL / 0 value means "off". */
typedef struct memhip_branch {
  const void* y; int64_t ldy;   /* bf16 [rows, D] branch output, NULL when dgamma is (see memhip_layerscale_grad) */
  const float* gamma;           /* layer scale [D], NULL = none */
  const float* rowmask;         /* stochastic depth as a keep mask per sample (0/1), NULL = off */
  float keep_prob;              /* 1 - drop_prob */
  int32_t rows_per_sample;
  void* dy; int64_t lddy;       /* bf16 out */
  float* dgamma; float* dbias;  /* f32 [D], ACCUMULATED; NULL = not wanted */
  const int32_t* out_map;       /* stochastic depth as WORK SKIPPING (timm drop_path, mem/modeling_finetune.py:42-53,187-188: nothing of a
                                   dropped sample's branch is computed): i32 [samples], sample -> its index among the samples the branch
                                   KEPT this step, or -1.  The kept samples' rows of dy are placed compactly (row out_map[s] *
                                   rows_per_sample + t) scaled by 1 / keep_prob; dropped samples are neither read nor written.  rowmask
                                   and y must be NULL.  NULL = identity */
  const memhip_dropout_t* dropout;  /* the branch had element-wise dropout (epilogue RESIDUAL_DROP in the forward): dy = bf16(dt * keep *
                                   scale * gamma) (dt after drop path; dt * keep * scale rounded once in fp32, then * gamma), dbias += sum dy,
                                   dgamma += sum dt * keep * scale * y.  The mask of the branch's site is regenerated (memhip_dropout_t, row =
                                   residual-stream row + row0); D % 8 == 0.  NULL = no dropout */
} memhip_branch_t;
typedef struct memhip_branch_bwd_args {
  const float* dx; int64_t lddx;   /* f32 [M, D], the gradient of the residual stream */
  int32_t M, D;                    /* M counts the rows of the residual stream (all samples) */
  memhip_branch_t branch;
} memhip_branch_bwd_args_t;
int memhip_branch_bwd(const memhip_branch_bwd_args_t* args, memhip_stream_t stream);
/* memhip_layernorm_bwd (accumulating, no row gather) fused with the memhip_branch_bwd that follows it in a block's backward:
 * the updated dres row is consumed in registers (one pass over the fp32 gradient stream less).  The LayerNorm fields are
 * memhip_layernorm_bwd's, `branch` is memhip_branch_bwd's with dx = dres; D <= 1024; R counts residual-stream rows. */
typedef struct memhip_ln_bwd_branch_args {
  const void* dy; int64_t lddy;    /* bf16 */
  const float* x; int64_t ldx;
  int32_t R, D;
  const float* gamma; const float* mean; const float* rstd;
  float* dres; int64_t lddres;
  float* dgamma; float* dbeta;
  const int32_t* in_map;           /* work skipping, as branch.out_map: which samples the LayerNorm'ed branch kept (dy / mean / rstd hold
                                      those samples only; the others get no LayerNorm gradient).  With either map branch.rowmask and
                                      branch.y must be NULL.  NULL = identity */
  memhip_branch_t branch;
} memhip_ln_bwd_branch_args_t;
int memhip_layernorm_bwd_branch(const memhip_ln_bwd_branch_args_t* args, memhip_stream_t stream);

/* Backward of the token assembly (mem/modeling_pretrain.py:101-108): dcls += dx[cls rows],
 * dmask_token += sum dx*w, dy bf16 [B*L, D] = bf16(dx*(1-w)); mask u8 [B*L]. */
int memhip_embed_bwd(const float* dx, int64_t lddx, const uint8_t* mask, int B, int L, int D,
                     void* dy_bf16, int64_t lddy, float* dcls, float* dmask_token, memhip_stream_t stream);

/* nn.CrossEntropyLoss()(logits, labels) + mlm_acc  (mem/engine_for_pretraining.py:152,233).
 * logits bf16 [M, V] (in place -> dlogits = (softmax - onehot) * grad_scale when write_grad);
 * row_loss f32 [M], row_correct i32 [M] scratch; out2 f32 [2] = {mean loss, accuracy}. */
int memhip_cross_entropy(void* logits_bf16, int64_t ld, const int64_t* labels, int M, int V,
                         float grad_scale, float* row_loss, int32_t* row_correct, int write_grad,
                         float* out2, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused attention with shared relative position bias, head_dim 64, <= 256 tokens
 * replaces Attention.forward q*scale .. (attn@v)   mem/modeling_finetune.py:137-154
 *          RelativePositionBias (index + forward)    mem/modeling_finetune.py:213-247
 * ------------------------------------------------------------------------
 * qkv    bf16 [B*T, 3D] token-major, columns [q*scale | k | v], head h at h*64
 * table  f32 [(2Wh-1)(2Ww-1)+3, heads] = relative_position_bias_table; T = Wh*Ww + 1 (cls first).
 *        The additive bias is gathered from the table on chip (bucket index computed
 *        arithmetically, identical to relative_position_index); no [heads,T,T] tensor is read.
 * out    bf16 [B*T, D];  lse f32 [B, heads, TP], TP = memhip_attn_tokens_padded(T) (for backward)
 * bwd:   delta f32 [(2*B*T + 4) * heads]: memhip_attn_delta fills [B*T, heads] = rowsum(dout * out)
 *        per head and, behind it, [B*T, heads] = |dout_row,head|^2; the last 4 * heads floats are
 *        scratch of memhip_attn_bwd (per-head bounds max |dout_row|^2, max |delta|, max |v_key|^2
 *        that scale the fixed-point buckets of the table gradient);
 *        dqkv bf16 [B*T, 3D] (dq already multiplied by `scale`);
 *        dtable f32 [num_rel, heads] += table gradient (NULL skips it);
 *        dq_bias / dv_bias f32 [D] += column sums of dq / dv (the q_bias / v_bias gradients).
 * memhip_relpos_gather materialises the bias tensor (tests / inspection only).
 */
int memhip_attn_tokens_padded(int T);
int memhip_relpos_gather(const float* table, const int32_t* index /*[T*T]*/, int T, int TP, int heads,
                         float* bias_pad, float* biasT_pad /*[heads,TP(key),TP(query)] or NULL*/,
                         memhip_stream_t stream);
int memhip_attn_fwd(const void* qkv, int64_t ldqkv, int B, int T, int D, int heads, const float* table,
                    int window_h, int window_w, void* out, int64_t ldo, float* lse, memhip_stream_t stream);
int memhip_attn_delta(const void* dout, const void* out, int64_t ldo, int64_t rows, int heads, float* delta,
                      memhip_stream_t stream);
/* Attention.forward backward (mem/modeling_finetune.py:137-154, RelativePositionBias :213-247).  Host struct, read at the call. */
typedef struct memhip_attn_bwd_args {
  const void* qkv; int64_t ldqkv;
  const void* dout; int64_t ldo;
  const void* out; int64_t ldout;  /* the forward OUTPUT (bf16 [B*T, D]): rowsum(dout * out) is computed by the library -- inside the fused
                                      14 x 14 kernel when that kernel applies (no separate pass over dout and out: 25 us per ViT-B layer at
                                      B = 256), otherwise by memhip_attn_delta into `delta` (then ldout == ldo is required).  NULL = the
                                      caller filled `delta` with memhip_attn_delta */
  const float* lse;
  float* delta;                    /* always the [(2*B*T + 4) * heads] workspace described above */
  const float* table;
  int32_t window_h, window_w, B, T, D, heads;
  float scale;
  int32_t reserved0;
  void* dqkv; int64_t lddqkv;
  float* dtable; float* dq_bias; float* dv_bias;
  void* ws; int64_t ws_bytes;      /* caller-owned scratch (round 6).  For the long windows the slot-layout kernels take (40 or 20 tokens wide,
                                      more than 256 tokens: BASELINE configs[4]) the backward then runs in its dS-storing form: the dK / dV
                                      kernel writes dS (bf16) to the workspace and owns the table gradient, the dQ kernel is a streaming
                                      product over it -- the score tile is computed once instead of twice.  memhip_attn_bwd_workspace returns
                                      the bytes that form wants (0: this shape has no such form); NULL, misaligned, too small or any other
                                      shape = the recomputing form.  Nothing is kept in it between calls.  Same outputs and rounding points
                                      either way (the table gradient is summed in another order: fixed-point buckets per workgroup, then
                                      float atomics) */
} memhip_attn_bwd_args_t;
int memhip_attn_bwd(const memhip_attn_bwd_args_t* args, memhip_stream_t stream);
int64_t memhip_attn_bwd_workspace(int B, int T, int heads, int window_h, int window_w);

/* The dispatch of memhip_attn_fwd / memhip_attn_bwd as data (additive to ABI 7): the kernel family, its template arguments,
 * the samples-per-workgroup numbers the kernels take and the ordered launches, auxiliary ones included.
 * memhip_attn_plan_fwd / _bwd validate the shape like the calls themselves and plan with the current option values for a
 * stream with stream_cus usable CUs; they launch nothing and need no device.  has_dtable / has_dv_bias: the call gives
 * dtable / dv_bias; has_out: the call gives the forward output; ws / ws_bytes: the call's workspace
 * (checked for NULL and alignment, never read).  A shape no family takes: MEMHIP_EUNSUPPORTED, as from the call. */
#define MEMHIP_ATTN_16 1        /* attn16.hip: the 14 x 14 window, fused backward */
#define MEMHIP_ATTN_SMALL 2     /* attn.hip: up to 256 tokens held on chip */
#define MEMHIP_ATTN_WIN 3       /* attn_win.hip: slot layout, windows 40 / 20 wide; backward recomputes the scores */
#define MEMHIP_ATTN_WIN_DS 4    /* attn_win.hip, backward only: the dS-storing pair over the caller's workspace */
#define MEMHIP_ATTN_STREAM 5    /* attn_stream.hip: any longer sequence */
enum { MEMHIP_ATTN_K_STATS_ZERO, MEMHIP_ATTN_K_DELTA, MEMHIP_ATTN_K_FWD, MEMHIP_ATTN_K_BWD_KV, MEMHIP_ATTN_K_BWD_Q,
       MEMHIP_ATTN_K_FWD16, MEMHIP_ATTN_K_BWD16,
       MEMHIP_ATTN_K_WIN_STATS, MEMHIP_ATTN_K_FWD_WIN, MEMHIP_ATTN_K_BWD_KV_WIN, MEMHIP_ATTN_K_BWD_Q_WIN,
       MEMHIP_ATTN_K_BWD_KVS_WIN, MEMHIP_ATTN_K_BWD_QS_WIN,
       MEMHIP_ATTN_K_FWD_STREAM, MEMHIP_ATTN_K_BWD_KV_STREAM, MEMHIP_ATTN_K_BWD_Q_STREAM };
typedef struct memhip_attn_launch {
  int32_t kernel;             /* MEMHIP_ATTN_K_* */
  int32_t grid_x, grid_y, grid_z;
  int32_t block;              /* workgroup size */
  int32_t lds;                /* dynamic LDS bytes */
} memhip_attn_launch_t;
typedef struct memhip_attn_plan {
  int32_t family;             /* MEMHIP_ATTN_* (0: nothing to do, B = 0) */
  int32_t n;                  /* SMALL: kernel template argument, 32-token blocks */
  int32_t ww;                 /* WIN / WIN_DS: kernel template argument, window width */
  int32_t vb, dt, fd;         /* backward template choices: v_bias gradient, table gradient, delta inside the kernel (ATTN_16) */
  int32_t spb;                /* SMALL: samples per workgroup */
  int32_t nwg;                /* ATTN_16: workgroups per head */
  int32_t groups;             /* WIN / WIN_DS / STREAM: workgroups per (head, sample): groups of 8 token blocks */
  int32_t nbz, nbq, nbs;      /* WIN / WIN_DS: sample slots of the grids (nbq: the kernel that owns the table gradient, nbs: the
                                 streaming dQ kernel of WIN_DS) */
  int32_t qgroups, qs;        /* WIN_DS: workgroups per (head, sample) of the streaming dQ kernel; slots per row of stored dS */
  int32_t stream_spb;         /* STREAM backward: samples per workgroup of the dQ kernel */
  int32_t lds_over;           /* internal: LDS bytes of the last family tried when none fits (the query fails instead) */
  int32_t count;
  memhip_attn_launch_t l[5];
} memhip_attn_plan_t;
int memhip_attn_plan_fwd(int B, int T, int D, int heads, int window_h, int window_w, int stream_cus, memhip_attn_plan_t* out);
int memhip_attn_plan_bwd(int B, int T, int D, int heads, int window_h, int window_w, int has_dtable, int has_dv_bias,
                         int has_out, const void* ws, int64_t ws_bytes, int stream_cus, memhip_attn_plan_t* out);

/* ------------------------------------------------------------------------
 * fp32 PARITY MODE (`--precision fp32`): the ViT path with fp32 operands / accumulation and no bf16 rounding points --
 * the reference's arithmetic without autocast (same reference lines as the bf16 entry points above).  For loss-curve
 * parity against the reference's fp32 CPU run (north star: step-100 loss within 1e-4); speed is secondary.
 * ------------------------------------------------------------------------
 * f32_gemm_nt: memhip_gemm_args_t with A, B, out0, out1 and (DGELU) aux as fp32; epilogues BIAS_BF16 (= plain bias,
 *   fp32 out), BIAS_GELU (exact erf), RESIDUAL, DGELU, F32, PATCH_EMBED; K and ld multiples of 4 (K is zero-extended to
 *   the next multiple of 32 inside).  f32_transpose: out [C, ldout] = in [R, C]^T, columns >= R zero.
 * f32_attn_*: generic attention (head_dim 32 or 64, T <= 256): bias[h,i,j] = table[index[i*T+j], h] (index NULL: none);
 *   bwd zeroes dqkv, then dq (times scale) by stores, dk / dv / dtable by fp32 atomics; delta = sum_j P dP. */
int memhip_f32_gemm_nt(const memhip_gemm_args_t* args, memhip_stream_t stream);
int memhip_f32_transpose(const float* in, int64_t ldin, int R, int C, float* out, int64_t ldout, memhip_stream_t stream);
int memhip_f32_layernorm_fwd(const float* x, int64_t ldx, const int32_t* row_idx, int R, int D, const float* gamma,
                             const float* beta, float eps, float* y, int64_t ldy, float* mean, float* rstd,
                             memhip_stream_t stream);
int memhip_f32_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const int32_t* row_idx, int R, int D,
                             const float* gamma, const float* mean, const float* rstd, float* dres, int64_t lddres,
                             int accumulate, float* dgamma, float* dbeta, memhip_stream_t stream);
int memhip_f32_branch_bwd(const float* dx, int64_t lddx, const float* y, int64_t ldy, const float* gamma, const float* rowmask,
                          float keep_prob, int rows_per_sample, int M, int D, float* dy, int64_t lddy, float* dgamma,
                          float* dbias, memhip_stream_t stream);
int memhip_f32_embed_bwd(const float* dx, int64_t lddx, const uint8_t* mask, int B, int L, int D, float* dy, int64_t lddy,
                         float* dcls, float* dmask_token, memhip_stream_t stream);
int memhip_f32_cross_entropy(float* logits, int64_t ld, const int64_t* labels, int M, int V, float grad_scale,
                             float* row_loss, int32_t* row_correct, int write_grad, float* out2, memhip_stream_t stream);
int memhip_f32_colsum(const float* in, int64_t ld, int R, int C, float* out, memhip_stream_t stream);
int memhip_f32_im2col(const float* x, int B, int C, int H, int W, int ph, int pw, float* out, memhip_stream_t stream);
int memhip_f32_attn_fwd(const float* qkv, int64_t ldqkv, int B, int T, int D, int heads, const float* table,
                        const int32_t* index, float* out, int64_t ldo, float* lse, memhip_stream_t stream);
int memhip_f32_attn_bwd(const float* qkv, int64_t ldqkv, const float* dout, int64_t ldo, int B, int T, int D, int heads,
                        float scale, const float* table, const int32_t* index, float* dqkv, int64_t lddqkv, float* dtable,
                        memhip_stream_t stream);

/* MAE variant (`--mae 1`), fp32 path: token plumbing and loss around the generic blocks above
 * replaces random_masking gather / mask-token unshuffle / forward_loss     mem/modeling_mae.py:204-292
 *   enc_assemble: out [B,(K+1),D]: row (b,0) = cls + pos[0]; row (b,1+j) = xe[b, ids_keep[b,j]] + pos[1 + ids_keep[b,j]]
 *   dec_assemble: out [B,(L+1),D]: row (b,0) = y[b,0] + dpos[0]; row (b,1+l) = (r < K ? y[b,1+r] : mask_token) + dpos[1+l],
 *                 r = ids_restore[b,l]
 *   *_bwd: the exact transposes (dxe is zeroed inside; dcls / dmask_token accumulate)
 *   mae_loss: pred [B,(L+1),p*p*C] (cls row ignored) vs patchify(img) ('nchpwq->nhwpqc'); row_loss [B,L] = per-patch mean
 *             squared error times its weight (only_masked: mask / sum(mask), else 1), dpred = gradient of the summed loss;
 *             scratch2[0] = sum(mask), scratch2[1] = loss. */
int memhip_mae_enc_assemble(const float* xe, const float* pos, const float* cls, const int64_t* ids_keep, int B, int L, int K,
                            int D, float* out, memhip_stream_t stream);
int memhip_mae_enc_assemble_bwd(const float* dx, const int64_t* ids_keep, int B, int L, int K, int D, float* dxe, float* dcls,
                                memhip_stream_t stream);
int memhip_mae_dec_assemble(const float* y, const float* mask_token, const float* dpos, const int64_t* ids_restore, int B, int L,
                            int K, int D, float* out, memhip_stream_t stream);
int memhip_mae_dec_assemble_bwd(const float* dxd, const int64_t* ids_restore, int B, int L, int K, int D, float* dy,
                                float* dmask_token, memhip_stream_t stream);
int memhip_mae_loss(const float* pred, const float* img, const float* mask, int B, int C, int H, int W, int patch,
                    int only_masked, float* row_loss, float* dpred, float* scratch2, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Frozen dVAE tokenizer forward
 * replaces DiscreteVAE.get_codebook_indices          eventvae/vae/vae_model.py:153-158
 *          encoder stack / ResBlock                   eventvae/vae/vae_model.py:29-42,86-101
 * called every pretraining step at                   mem/engine_for_pretraining.py:144
 * ------------------------------------------------------------------------
 * Three modes (MEMHIP_CONV_*), one set of entry points.  conv2d: out = [relu](conv(in, weight) + bias) [+ add] on NHWC
 * activations with a one-pixel zero border, [B, H+2, W+2, C] (the caller zeroes the buffers once; the kernels only write
 * interiors); weight [C_out, k*k*C_in] packed (ky, kx, c)-major; `add` has the layout of `out` (ResBlock residual).
 *
 * MEMHIP_CONV_BF16: activations and weights bf16, fp32 accumulate (the reference runs this stage in fp32 / TF32).  Shapes
 * 4x4/s2/p1, 3x3/s1/p1, 1x1/s1/p0; C_in = 4 (first layer: 3 channels + 1 zero, 4x4 only) or a multiple of 64; C_out a
 * multiple of 8.
 *
 * MEMHIP_CONV_F32 -- the EXACT-label mode (default): the reference computes the tokenizer in fp32
 * (mem/engine_for_pretraining.py:140-145 is outside the autocast block at :147) and its output is an integer, so the
 * labels are produced with fp32 operands and fp32 accumulation (v_mfma_f32_16x16x4_f32, an fmaf chain over k).
 * Activations and weights fp32; any kernel size 1..4, stride >= 1, pad 0/1; C_in, C_out multiples of 4, k*k*C_in a
 * multiple of 32.
 *
 * MEMHIP_CONV_F16X2 -- "fp16 x 2" (opt-in, `--tokenizer_impl hip_fp16x2`): every fp32 value travels as two fp16 planes
 * hi = fp16(v), lo = fp16((v - hi) * 2048); a product is three fp16 MFMAs (hi*hi + (hi*lo + lo*hi) / 2048, exact products,
 * fp32 accumulation).  Logits within 1.4e-5 of the fp32 module at a spread of 1.77 (between the exact fp32 mode and the bf16
 * mode), ~2x faster than fp32.  Tensors: base pointer of the hi plane + plane stride to the lo plane; weights
 * [2][C_out, k*k*C_in]; shapes as MEMHIP_CONV_BF16.
 *
 * A field that the mode does not have must be 0 / NULL (MEMHIP_EINVAL otherwise); B == 0 is MEMHIP_OK, nothing is read. */
enum { MEMHIP_CONV_BF16, MEMHIP_CONV_F32, MEMHIP_CONV_F16X2 };
typedef struct memhip_conv_args {
  int32_t mode;               /* MEMHIP_CONV_* */
  int32_t reserved0;
  const void* in;             /* [B, H+2, W+2, Cin] */
  int64_t in_plane;           /* the four *_plane: MEMHIP_CONV_F16X2 only, elements from the hi plane to the lo plane */
  const void* weight;         /* [Cout, ksize*ksize*Cin] */
  int64_t w_plane;
  const float* bias;          /* f32 [Cout], or NULL */
  const void* add;            /* residual, laid out like `out`, or NULL */
  int64_t add_plane;
  void* out;                  /* [B, Ho+2, Wo+2, Cout] interior, or see out_padded / out_f32 */
  int64_t out_plane;
  int32_t B, H, W, Cin, Cout, ksize, stride, pad;
  int32_t relu;
  int32_t out_padded;         /* 0: `out` is a dense [B*Ho*Wo, Cout] matrix (the token logits) */
  int32_t out_f32;            /* MEMHIP_CONV_F16X2 only: `out` is the dense fp32 logit matrix (out_padded = 0, out_plane unused) */
  int32_t reserved1;
  const int32_t* n_active;    /* MEMHIP_CONV_F32 only; NULL = static batch.  Device int32: only the first *n_active samples
                                 of the capacity B are live (the grid covers the capacity; tiles behind the live rows return at once) */
} memhip_conv_args_t;
int memhip_conv2d_nhwc(const memhip_conv_args_t* args, memhip_stream_t stream);
/* x f32 NCHW [B, C<=4, H, W] -> the interior of `out` [B, H+2, W+2, 4] in the activation format of `mode` (out_plane:
 * MEMHIP_CONV_F16X2 only, else 0); mean/std f32 [C] or both NULL (DiscreteVAE.norm) */
int memhip_nchw_to_padded_nhwc4(const float* x, int B, int C, int H, int W, const float* mean, const float* stdv, void* out,
                                int64_t out_plane, int mode, memhip_stream_t stream);
/* ids i64 [M] = argmax over the N columns of logits [M, ld] (first maximum; a NaN is the greatest).  mode = the logits' type:
 * MEMHIP_CONV_BF16 (N, ld multiples of 8; top2_gap, row_rms, n_samples NULL) or MEMHIP_CONV_F32 (multiples of 4; the
 * fp16x2 mode's logits are fp32 too).  fp32, each may be NULL: top2_gap f32 [M] = best - runner-up logit, row_rms f32 [M] =
 * sqrt(mean_n logit^2); with n_samples (device int32) only the first *n_samples x rows_per_sample rows exist. */
int memhip_argmax_rows(const void* logits, int mode, int64_t ld, int M, int N, int64_t* ids, float* top2_gap, float* row_rms,
                       const int32_t* n_samples, int rows_per_sample, memhip_stream_t stream);

/* Certified split-precision tokenizer (round 5; replaces the same reference lines: eventvae/vae/vae_model.py:153-158, called
 * at mem/engine_for_pretraining.py:139-145 in fp32).  The fp16x2 convolutions produce the logits; a label is ACCEPTED
 * only where its top-2 gap exceeds kappa x the row's rms (kappa = twice a stated bound on the fp16x2 logit deviation relative
 * to the row rms: then the fp32 argmax is the same index); every sample that holds a token below the margin is recomputed
 * on the fp32 path (memhip_conv_args_t.n_active, memhip_argmax_rows' n_samples) and its labels are replaced.  Everything is
 * decided on the device (no host synchronisation):
 *   tok_flag_samples     list (int32 [B]) = indices of the samples with a token whose gap is not > kappa x rms (ascending),
 *                        count[0] = their number; stats (int64 [2], may be NULL): += flagged samples, += 1 call
 *   tok_gather_images_f32  the fp32 nchw_to_padded_nhwc4 of the samples list[offset + j], j < n_round[0] = clamp(count - offset, 0, R)
 *                        into slots 0.. of `out` (n_round is written: the dynamic batch of the round)
 *   tok_scatter_ids      ids_out[list[offset + j] * tokens_per_sample + t] = ids_in[j * tokens_per_sample + t], j < *n_round */
int memhip_tok_flag_samples(const float* top2_gap, const float* row_rms, int B, int tokens_per_sample, float kappa,
                            int32_t* list, int32_t* count, int64_t* stats, memhip_stream_t stream);
int memhip_tok_gather_images_f32(const float* x, int C, int H, int W, const float* mean, const float* stdv,
                                 const int32_t* list, const int32_t* count, int offset, int R, float* out, int32_t* n_round,
                                 memhip_stream_t stream);
int memhip_tok_scatter_ids(const int64_t* ids_in, const int32_t* list, const int32_t* n_round, int offset, int R,
                           int tokens_per_sample, int64_t* ids_out, memhip_stream_t stream);

/* The dispatch of memhip_conv2d_nhwc as data: the layer's geometry and the ordered launches.  memhip_conv_plan takes the
 * struct of the call and validates it like the call (same messages, same return codes), except that in / weight / out may be
 * NULL: no pointer is dereferenced, `add` and `n_active` only say whether the call has a residual / a dynamic batch (two
 * launches, of which the one whose [dyn_lo, dyn_hi) holds *n_active works).  It plans with the current value of the
 * "conv_waves" option for a device of device_cus CUs (< 0: the current device's); it launches nothing and needs no device
 * when device_cus is given. */
enum { MEMHIP_CONV_K_BF16,          /* conv_gemm_kernel */
       MEMHIP_CONV_K_F32,           /* conv_gemm_f32_kernel: 128-row tiles */
       MEMHIP_CONV_K_F32_M32,       /* conv_gemm_f32_m32_kernel: 32-row tiles, dynamic batch only */
       MEMHIP_CONV_K_F16X2_W4,      /* conv_gemm_f16x2_kernel<4> */
       MEMHIP_CONV_K_F16X2_W8,      /* conv_gemm_f16x2_kernel<8> */
       MEMHIP_CONV_K_F16X2_WIDE,    /* conv_gemm_f16x2_wide_kernel: 256 x 128 tile */
       MEMHIP_CONV_K_F16X2_FIRST,   /* conv_gemm_f16x2_first_kernel: C_in = 4, persistent */
       MEMHIP_CONV_K_BF16_T };      /* convt_gemm_kernel: the decoder's transposed convolution (memhip_convt_plan only) */
typedef struct memhip_conv_launch {
  int32_t kernel;             /* MEMHIP_CONV_K_* */
  int32_t grid;               /* workgroups */
  int32_t block;              /* workgroup size */
  int32_t lds;                /* dynamic LDS bytes */
  int32_t dyn_lo, dyn_hi;     /* dynamic batch: works when dyn_lo <= *n_active < dyn_hi (otherwise 0, 2^30) */
} memhip_conv_launch_t;
typedef struct memhip_conv_plan {
  int32_t Hp, Wp, Ho, Wo;     /* padded input, output */
  int32_t K, off;             /* GEMM depth k*k*C_in; first tap = 1 - pad */
  int64_t M;                  /* GEMM rows B*Ho*Wo (0: nothing to do) */
  int32_t count;
  memhip_conv_launch_t l[2];
} memhip_conv_plan_t;
int memhip_conv_plan(const memhip_conv_args_t* args, int device_cus, memhip_conv_plan_t* out);

/* ------------------------------------------------------------------------
 * dVAE tokenizer, decoder side and evaluation (additive at ABI 10: plain arguments; at the next ABI bump these belong in an
 * args struct like memhip_conv_args_t, one for the call and the plan query)
 * replaces nn.ConvTranspose2d(4, stride 2, padding 1)  eventvae/vae/vae_model.py:92
 *          DiscreteVAE.decode                           eventvae/vae/vae_model.py:160-171
 *          the KL term of the dVAE loss / evaluate      eventvae/vae/vae_model.py:203-206 (evaluate: :216-266)
 * ------------------------------------------------------------------------
 * memhip_convt2d_nhwc: out = [relu](conv_transpose(in, W, stride 2, padding 1) + bias), bf16 operands, fp32 accumulation, on
 * the tokenizer's activation format: in bf16 [B, H+2, W+2, Cin] with a zero border -> the INTERIOR of out bf16
 * [B, 2H+2, 2W+2, Cout] (the border ring is never written; the caller zeroes the buffer once).  Four output phases (py, px),
 * each a 2x2-tap stride-1 implicit GEMM (M = B*H*W, K = 4*Cin, N = Cout), one launch:
 *   out[b, 2y+py, 2x+px, co] = bias[co] + sum_{dy,dx in {0,1}} sum_ci in_pad[b, y+py+dy, x+px+dx, ci] * W[ci, co, 3-py-2dy, 3-px-2dx]
 * weight: bf16 [4 (phase = 2 py + px)][Cout][(dy, dx, ci)] packed on the host from torch's [Cin, Cout, 4, 4]
 * (mem_amd pack_convt_weight); bias f32 [Cout] or NULL.  Cin a multiple of 64, Cout a multiple of 8; B == 0 is MEMHIP_OK.
 * memhip_convt_plan: the dispatch of that call as data (Hp, Wp of the input, Ho = 2H, Wo = 2W, K = 4*Cin, off = 0,
 * M = B*H*W, one launch MEMHIP_CONV_K_BF16_T of 4 x tiles workgroups); validates like the call (same codes and messages,
 * pointers aside), launches nothing and needs no device. */
int memhip_convt2d_nhwc(const void* in, const void* weight, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                        int relu, memhip_stream_t stream);
int memhip_convt_plan(int B, int H, int W, int Cin, int Cout, int device_cus, memhip_conv_plan_t* out);
/* row_kl f32 [M]: KL(softmax(logits[m]) || uniform) = sum_n q log q + log N over the N columns of logits [M, ld], in one pass
 * over the row (no [M, N] log_softmax matrix); mode = the logits' type as in memhip_argmax_rows: MEMHIP_CONV_BF16 (N, ld
 * multiples of 8) or MEMHIP_CONV_F32 (multiples of 4).  The reference's 'batchmean' kl_div is sum(row_kl) / batch size. */
int memhip_kl_uniform_rows(const void* logits, int mode, int64_t ld, int M, int N, float* row_kl, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * dVAE tokenizer, training side: the weight gradient of every convolution of the model (additive at ABI 10)
 * replaces autograd's weight gradients of  ResBlock's Conv2d(3,1,1) / Conv2d(1)           eventvae/vae/vae_model.py:29-41
 *                                          Conv2d(4,2,1), ConvTranspose2d(4,2,1), heads  eventvae/vae/vae_model.py:86-102
 * ------------------------------------------------------------------------
 * memhip_conv_wgrad_nhwc: one implicit TN GEMM, the reduction over the pixels (b, y, x) of the SMALL grid Hs x Ws:
 *   G[n, (ky, kx, c)] (+)= sum_{b,y,x} Small[b, y, x, n] * BigPad[b, s*y + ky + 1 - pad, s*x + kx + 1 - pad, c]
 * grad   f32 [N, k*k*C], (ky, kx, c)-major: the packed layout of the forward weight (memhip_conv2d_nhwc's [Cout, k*k*Cin]).
 * small  bf16, N channels over Hs x Ws: the one-pixel-border format [B, Hs+2, Ws+2, N] (small_padded = 1; its ring is never
 *        read) or the dense matrix [B*Hs*Ws, N] (small_padded = 0), rows (b, y, x).
 * big    bf16 [B, s*Hs + 2, s*Ws + 2, C], always the padded format; its ring IS read and must be zero.
 * Forms (ksize, stride, pad): (4, 2, 1), (3, 1, 1), (1, 1, 0).  C = 4 (4x4 only: the first encoder layer) or a multiple of 8;
 * N a multiple of 8.  small and big 16-byte aligned.
 *   Conv2d:                  small = the gradient of the pre-activation, big = the layer's input, G = dW packed.
 *   ConvTranspose2d(4,2,1):  small = the layer's INPUT [.., Cin], big = the gradient of its output [B, 2H+2, 2W+2, Cout]:
 *                            torch's dW[ci, co, ky, kx] = G[ci, (ky, kx, co)].
 *   The two 1x1 heads:       small dense (token logits [M, num_tokens], reconstruction [M, 8]).
 * The pixel range is split over the grid (memhip_conv_wgrad_plan_t.splits slices of whole 64-pixel stages).  No atomics: with
 * more than one slice every workgroup stores its partial tile into `workspace` ([splits][N][K] f32, all of it overwritten) and
 * a second launch folds the slices in ascending order into grad (accumulate: onto what grad holds); two calls give the same
 * bits.  One slice writes grad itself and needs no workspace.  workspace_bytes < the plan's ws_bytes: MEMHIP_EWORKSPACE.
 * memhip_conv_wgrad_plan: the dispatch as data for a device of device_cus CUs (< 0: the current device's, as the call uses);
 * it validates like the call (same codes and messages; pointers, alignment and the workspace size aside), launches nothing
 * and needs no device.  memhip_conv_wgrad_workspace: the plan's ws_bytes (0 for a rejected struct).
 * (The two structs are declared tag first, typedef second.) */
struct memhip_conv_wgrad_args {
  const void* small;          /* bf16, see above */
  const void* big;            /* bf16 padded, zero ring */
  float* grad;                /* f32 [N, ksize*ksize*C] */
  void* workspace;            /* >= plan.ws_bytes, 16-byte aligned; may be NULL when the plan has one slice */
  size_t workspace_bytes;
  int32_t B, Hs, Ws;          /* the SMALL pixel grid; big's is stride*Hs x stride*Ws */
  int32_t C, N;               /* channels of big / of small */
  int32_t ksize, stride, pad;
  int32_t small_padded;       /* 1: padded NHWC, 0: dense rows */
  int32_t accumulate;         /* 1: grad += , 0: grad = */
};
typedef struct memhip_conv_wgrad_args memhip_conv_wgrad_args_t;
struct memhip_conv_wgrad_plan {
  int64_t M;                  /* B*Hs*Ws reduction rows */
  int64_t ws_bytes;           /* splits > 1: splits * N * K * 4, else 0 */
  int32_t K;                  /* ksize*ksize*C columns of grad */
  int32_t Hbp, Wbp;           /* padded size of big */
  int32_t tiles_n, tiles_k;   /* 128 x 128 output tiles */
  int32_t splits, rows_per_split;   /* slices of the pixel range: slice i covers [i * rows_per_split, min(M, (i+1) * ...)) */
  int32_t grid, block, lds_bytes;   /* the GEMM launch: tiles_n * tiles_k * splits workgroups */
  int32_t fold_grid;          /* workgroups of the fold launch (256 threads), 0 with one slice */
  int32_t reserved;
};
typedef struct memhip_conv_wgrad_plan memhip_conv_wgrad_plan_t;
int memhip_conv_wgrad_nhwc(const memhip_conv_wgrad_args_t* args, memhip_stream_t stream);
int memhip_conv_wgrad_plan(const memhip_conv_wgrad_args_t* args, int device_cus, memhip_conv_wgrad_plan_t* out);
size_t memhip_conv_wgrad_workspace(const memhip_conv_wgrad_args_t* args, int device_cus);
/* ReLU backward in place, with the bias gradient: g *= (y > 0) over the R = B*H*W pixels of a bf16 buffer of C channels
 * (C % 8 == 0; padded = 1: g and y in the one-pixel-border format [B, H+2, W+2, C], rings untouched; 0: dense [R, C]);
 * y NULL: no mask.  colsum f32 [C] or NULL: (+)= the column sums of the masked g -- per-workgroup partial sums as plain
 * stores into `workspace` (memhip_relu_bwd_colsum_workspace bytes), folded in ascending order by a second launch: no
 * atomics, two calls give the same bits.  R == 0 is MEMHIP_OK. */
int memhip_relu_bwd_colsum(void* g, const void* y, int padded, int B, int H, int W, int C, float* colsum, int accumulate,
                           void* workspace, size_t workspace_bytes, memhip_stream_t stream);
size_t memhip_relu_bwd_colsum_workspace(int B, int H, int W, int C);

/* ------------------------------------------------------------------------
 * Layout / dtype movers
 * ------------------------------------------------------------------------ */
int memhip_cast_f32_bf16(const float* in, void* out_bf16, int64_t n, memhip_stream_t stream);
/* Zero fills of the training step (the reference: optimizer.zero_grad(), mem/engine_for_pretraining.py:160; torch.zeros
 * temporaries of autograd): `bytes` at p, or n ranges {byte offset, byte count} (device array of 2n int64, every value a
 * multiple of 16, total_bytes = their sum: it sizes the grid) relative to base, in one launch -- e.g. every gradient that is
 * accumulated by atomics, while the weight matrices are written, not accumulated, by the weight-gradient GEMM. */
int memhip_zero(void* p, int64_t bytes, memhip_stream_t stream);
int memhip_zero_ranges(void* base, const int64_t* ranges, int n, int64_t total_bytes, memhip_stream_t stream);
/* dst[s] = src[s] for the n listed samples s = ids[k] (n_per_sample fp32 values each, a multiple of 4): the residual rows of
 * the samples a stochastic-depth branch dropped (mem/modeling_finetune.py:187-188 with a zero keep mask) */
int memhip_copy_samples_f32(const float* src, float* dst, const int32_t* ids, int n, int64_t n_per_sample,
                            memhip_stream_t stream);
/* out bf16 [Cc, ldout] = in f32 [R, Cc]^T (the [in,out]-major copy of a Linear weight used by dgrad) */
int memhip_transpose_cast_f32_bf16(const float* in, int64_t ldin, int R, int Cc, void* out_bf16,
                                   int64_t ldout, memhip_stream_t stream);
/* n weight transposes (fp32 [R,C] -> bf16 [C, ldout], rows beyond R zero-filled up to min(ldout, 64-padded R))
 * in one launch: desc = device array of n records {const float* in; int64 ldin; int64 R; int64 C; bf16* out;
 * int64 ldout} (48 bytes each), tile_prefix = device i32 [n+1] with the first 64x64 tile index of every matrix
 * (tile_prefix[n] = total_tiles).  Same result as n calls of memhip_transpose_cast_f32_bf16.
 * The descriptors live on the device, so the entry cannot validate them.  Preconditions on every record, which the
 * kernel's 16-byte stores rely on: ldout % 8 == 0 and ldout >= R, and `out` 16-byte aligned.  (`in` and ldin are free:
 * a source that is not 16-byte aligned, or ldin % 4 != 0, takes the scalar load path.)  A launch on a slice
 * desc + k0 takes a tile_prefix that starts at 0 for record k0. */
int memhip_transpose_cast_batched(const void* desc, const int32_t* tile_prefix, int n, int total_tiles,
                                  memhip_stream_t stream);

/* out bf16 [Cc, ldout] = in bf16 [R, Cc]^T, columns [R, R_pad) zero-filled (R_pad % 64 == 0);
 * optional fused column sums of `in` (Linear bias gradients) over two column ranges. */
int memhip_transpose_bf16(const void* in, int64_t ldin, int R, int Cc, void* out, int64_t ldout, int R_pad,
                          float* colsum0, int c0_begin, int c0_end, float* colsum1, int c1_begin,
                          int c1_end, memhip_stream_t stream);
/* im2col of the k=s=patch conv (mem/modeling_finetune.py:203-209): x f32 [B,C,H,W] ->
 * bf16 [B*L, C*ph*pw], k = c*ph*pw + py*pw + px */
int memhip_im2col_bf16(const float* x, int B, int C, int H, int W, int ph, int pw, void* out_bf16,
                       memhip_stream_t stream);
/* x[b*T, :] = cls_token (mem/modeling_pretrain.py:101,108) */
int memhip_fill_cls(float* x, int64_t ldx, int B, int T, int D, const float* cls, memhip_stream_t stream);
/* y[n] += sum_k W[n,k] x[k]  (W bf16 [N, ldw], x f32 [K], y f32 [N]); optionally x_acc[k] += x[k] and
 * zero[k] = 0 (K floats each, may be NULL; `zero` must not alias x).  Used for the v_bias gradient:
 * sum over keys of dV = sum over queries of d(attn_out) (softmax rows sum to one) = (column sums of the
 * proj-output gradient) @ W_proj, so v_bias.grad is one 768x768 GEMV per block (modeling_finetune.py:128-139). */
int memhip_gemv_bf16_acc(const void* W, int64_t ldw, int N, int K, const float* x, float* y, float* x_acc,
                         float* zero, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Optimizer step on flat fp32 buffers (tensors padded to 1024 elements)
 * replaces clip_grad_norm_ / get_grad_norm_   mem/utils.py:360-366,380-392
 *          optim.AdamW(betas=(0.9,0.95))      mem/optim_factory.py:121,132-133
 * ------------------------------------------------------------------------ */
size_t memhip_grad_norm_workspace(void);
int memhip_grad_norm(const float* g, int64_t n, float* norm_out, void* workspace, size_t workspace_bytes,
                     memhip_stream_t stream);
/* wd_flag_per_chunk u8 [n/1024]: 1 = weight decay applies to that chunk.  gnorm (device scalar) and
 * max_norm > 0 fold gradient clipping into the update; step >= 1 is the AdamW step count. */
int memhip_adamw(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* wd_flag_per_chunk,
                 double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                 const float* gnorm, double max_norm, memhip_stream_t stream);

/* The same step with per-group learning rates / weight decay (layer-wise lr decay of finetuning:
 * replaces get_parameter_groups + LayerDecayValueAssigner   mem/optim_factory.py:31-100 feeding optim.AdamW).
 * group_of_chunk u8 [n/1024]; group_table f32 [n_groups][2] (device) = {1 - lr_g*wd_g, lr_g / (1 - beta1^step)},
 * computed by the caller in double and rounded once, like torch's Python-side scalars.
 * Precondition the entry cannot check (group_of_chunk lives on the device): every group_of_chunk[c] < n_groups; a
 * larger id reads beyond the table.  A group {1, 0} is frozen: its parameters keep their bits, its moments still move. */
int memhip_adamw_groups(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* group_of_chunk,
                        const float* group_table, int n_groups, double beta1, double beta2, double eps, int step,
                        const float* gnorm, double max_norm, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Finetuning recipe around the ViT step (finetune_recipe.hip)
 * replaces timm.data.Mixup (mixup 0.8 / cutmix 1.0)                  mem/run_class_finetuning.py:504-511
 *          timm.loss.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy   mem/run_class_finetuning.py:609-613
 *          timm.utils.ModelEma.update                                 mem/run_class_finetuning.py:519-527, mem/engine_for_finetuning.py:127-128
 * ------------------------------------------------------------------------
 * mixup: x f32 [B, C, H, W] mixed IN PLACE with the flipped batch as it was before the call (sample i with sample B-1-i):
 *   lam f32 [B], box i32 [B, 4] = (yl, yh, xl, xh) per sample (device).  A box without area: out[i] = lam[i] * x[i] +
 *   (1 - lam[i]) * x[B-1-i] (lam[i] == 1: sample i is left untouched bit for bit); otherwise out[i] = x[B-1-i] inside the box
 *   and x[i] outside it (exact copies).  One work-item owns the same elements of both samples of a pair, so no scratch copy of
 *   the batch exists; 16-byte accesses when C*H*W is a multiple of 4 and x is 16-byte aligned (any shape otherwise).
 *   lam_host / box_host (host, may be NULL): the same values, validated BEFORE the launch (lam in [0, 1],
 *   0 <= yl <= yh <= H, 0 <= xl <= xh <= W) -- the parameters are drawn on the host, the device arrays are never read back. */
int memhip_mixup(float* x, int B, int C, int H, int W, const float* lam, const int32_t* box, const float* lam_host,
                 const int32_t* box_host, memhip_stream_t stream);
/* timm.data.mixup.mixup_target: t f32 [B, V] (leading dimension ldt), t[i] = lam[i] * onehot(labels[i]) +
 * (1 - lam[i]) * onehot(labels[B-1-i]), one-hot values off = smoothing / V and on = 1 - smoothing + off.  A label outside
 * [0, V) is never used as an index; its row (and its partner's) is NaN, which the training loop's non-finite-loss stop reports. */
int memhip_mix_targets(const int64_t* labels, const float* lam, int B, int V, double smoothing, float* t, int64_t ldt,
                       memhip_stream_t stream);
/* Cross-entropy against soft targets; logits [M, V] bf16 (logits_f32 = 0) or fp32 (1), ANY 2 <= V <= 8192, leading dimension ld.
 *   target f32 [M, V] (ldt) given, labels NULL:   loss_r = -sum_c t_rc * log_softmax(x_r)_c           (SoftTargetCrossEntropy)
 *   labels i64 [M] given, target NULL:            loss_r = (1 - s) * nll_r + s * mean_c(-log_softmax(x_r)_c), s = smoothing
 *                                                 (LabelSmoothingCrossEntropy; no dense target is built; label outside [0, V): NaN)
 * row_loss f32 [M], row_correct i32 [M] scratch; out2 f32 [2] = {mean loss, top-1 accuracy against the label / argmax_c t};
 * write_grad: dlogits (dtype of the logits, leading dimension lddl, may BE the logits) = grad_scale * (softmax * sum_c t_rc - t_r). */
int memhip_ce_soft(const void* logits, int logits_f32, int64_t ld, const float* target, int64_t ldt, const int64_t* labels,
                   float smoothing, int M, int V, float grad_scale, void* dlogits, int64_t lddl, float* row_loss,
                   int32_t* row_correct, int write_grad, float* out2, memhip_stream_t stream);
/* ema[i] = decay * ema[i] + (1 - decay) * p[i] over n fp32 values (16-byte aligned buffers, any n): decay and 1 - decay are
 * each rounded to fp32 from the double (timm's arithmetic: Python scalars times fp32 tensors), the update is fp32. */
int memhip_ema_update(float* ema, const float* p, int64_t n, double decay, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Token pooling of the finetuning head (pool.hip)
 * replaces t[:, 1:, :].mean(1) in front of fc_norm                     mem/modeling_finetune.py:349-354
 * ------------------------------------------------------------------------
 * x f32 [B*T, ldx] (the residual stream, sample-major, ldx >= D), out f32 [B, D]:
 *   out[b] = (sum over t = 1 .. T-1 of x[b*T + t]) / (T - 1)        (row 0 of a sample, the cls token, is skipped)
 * fp32 accumulation in a fixed order (bit-reproducible), one read of x, no workspace, no atomics; T >= 2, any D
 * (16-byte lane loads when D and ldx are multiples of 4 and both buffers are 16-byte aligned). */
int memhip_pool_tokens(const float* x, int64_t ldx, int B, int T, int D, float* out, memhip_stream_t stream);
/* Its backward: dx f32 [B*T, D] (dense), dx[b*T + t] = dout[b] / (T - 1) for t >= 1 (IEEE division) and 0 for t = 0;
 * every element of dx is written. */
int memhip_pool_tokens_bwd(const float* dout, int B, int T, int D, float* dx, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense per-block feature maps (dense.hip; additive to ABI 7)
 * replaces x[:, 1:, :].permute(0, 2, 1).reshape(B, -1, Hp, Wp).contiguous()   mem/semantic_segmentation/backbone/mem.py:439-441
 *          (and its autograd backward); the streams of get_intermediate_layers  mem/modeling_finetune.py:361-378
 * ------------------------------------------------------------------------
 * x f32 [B*T, ldx] (the residual stream, sample-major, ldx >= D), out f32 [B, D, T-1] contiguous (= [B, D, Hp, Wp]):
 *   out[b, d, l] = x[b*T + 1 + l, d]   for the samples b0 <= b < b1    (row 0 of a sample, the cls token, is skipped)
 * A batched [L, D] -> [D, L] transpose through a padded LDS tile, 16-byte lane accesses and whole 128-byte lines on both
 * sides; samples outside [b0, b1) are neither read nor written.  T >= 2, D % 64 == 0, ldx % 4 == 0, x 16-byte aligned; any
 * T (the map side moves 16 bytes per lane when (T-1) % 4 == 0 and `out` is 16-byte aligned, 4 otherwise); at most 65535
 * samples per call. */
int memhip_tokens_to_maps(const float* x, int64_t ldx, int b0, int b1, int T, int D, float* out, memhip_stream_t stream);
/* Its backward INTO a gradient that already holds other terms: dx f32 [B*T, lddx], dmap f32 [B, D, T-1] contiguous:
 *   dx[b*T + 1 + l, d] += dmap[b, d, l]   for b0 <= b < b1
 * exactly one fp32 add per element, no atomics (every dx element has one writer: the result is deterministic); cls rows,
 * columns >= D and other samples are untouched.  Same shape rules (dx 16-byte aligned, lddx % 4 == 0). */
int memhip_maps_to_tokens_add(const float* dmap, int b0, int b1, int T, int D, float* dx, int64_t lddx, memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Feature-pyramid necks of the segmentation backbone (necks.hip; additive to ABI 8)
 * replaces fpn1 = ConvTranspose2d(2,2) -> SyncBatchNorm -> GELU -> ConvTranspose2d(2,2) and fpn2 = ConvTranspose2d(2,2)
 *          (and their autograd backward) around the bf16 GEMMs              mem/semantic_segmentation/backbone/mem.py:331-346
 * ------------------------------------------------------------------------
 * A ConvTranspose2d with kernel = stride = 2 is Y = X W: pixel rows X [R, D] (row = (b, y, x)), the weight [D, D, 2, 2] read
 * as the [D, 4D] matrix it is in memory (column 4 co + q, q = 2i + j).  Y [R, 4D] is INTERLEAVED: row r holds the four
 * output pixels (2y + i, 2x + j) of input pixel r per channel; as plain rows the same values are Z [4R, D],
 * Z[4r + q, co] = Y[r, 4 co + q].  A second level nests: row 16 r0 + 4 qa + qb is pixel (4y + 2ia + ib, 4x + 2ja + jb).
 * All bf16 buffers are dense and 16-byte aligned, D % 64 == 0; every kernel is pure streaming through a 64 x 64 LDS tile,
 * 16-byte lane accesses (8 on the fp32 side of level 1), ragged last tiles neither read nor written; no atomics.
 *
 * memhip_neck_maps_to_rows: map f32 [B, D, 2^level Hp, 2^level Wp] -> bf16 (round to nearest even),
 *   level 0: plain rows [B Hp Wp, D]; level 1 / 2: interleaved [B Hp Wp 4^(level-1), 4D] in the nested order above (the
 *   gradient of an upsampled map as the A operand of the dgrad / wgrad products).  map: 4- / 8- / 16-byte aligned at level
 *   0 / 1 / 2 (level 0 moves 16 bytes per lane when Hp Wp % 4 == 0 and map is 16-byte aligned, single floats otherwise).
 * memhip_neck_rows_to_maps: the inverse, bf16 -> f32 (exact). */
int memhip_neck_maps_to_rows(const float* map, int B, int D, int Hp, int Wp, int level, void* rows_bf16, memhip_stream_t stream);
int memhip_neck_rows_to_maps(const void* rows_bf16, int B, int D, int Hp, int Wp, int level, float* map, memhip_stream_t stream);
/* Column sums in two stages: at most MEMHIP_NECK_GROUPS partials per channel, stored to `workspace`
 * (memhip_neck_sums_workspace(D) bytes) and added by a finish kernel in fixed order (bit-reproducible).
 * memhip_neck_colstats: y bf16 [R, 4D] interleaved, shift f32 [D] -> out f32 [3, D] = count (4R), sum (x - shift),
 *   sum (x - shift)^2 per channel: with shift near the channel mean (the convolution's bias) the variance
 *   sum2 / n - (sum / n)^2 keeps its digits under a common offset.  The longest chain of fp32 additions behind one output is
 *   4 ceil(R / (8 G)) + 8 + G with G = min(ceil(R / 8), MEMHIP_NECK_GROUPS). */
#define MEMHIP_NECK_GROUPS 128
size_t memhip_neck_sums_workspace(int D);
int memhip_neck_colstats(const void* y_bf16, int64_t R, int D, const float* shift, float* workspace, size_t workspace_bytes,
                         float* out, memhip_stream_t stream);
/* z bf16 [4R, D] = bf16(gelu(gamma (y - mean) rstd + beta)) (fp32 chain, exact-erf GELU, one rounding), y bf16 [R, 4D]
 * interleaved; mean / rstd are the batch statistics in train() and the running ones in eval(). */
int memhip_neck_bn_gelu_fwd(const void* y_bf16, int64_t R, int D, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, void* z_bf16, memhip_stream_t stream);
/* Backward of the above from da bf16 [4R, D] (gradient w.r.t. z) and the stored y: with xhat = (y - mean) rstd,
 * u = gamma xhat + beta, g = da gelu'(u):
 *   _sums:  out f32 [2, D] = sum g (= dbeta), sum g xhat (= dgamma) per channel
 *   _apply: dy bf16 [R, 4D] interleaved = gamma rstd (g - sums[0] inv_n - xhat sums[1] inv_n); inv_n = 1 / (elements per
 *           channel over all ranks), sums = the (all-reduced) output of _sums. */
int memhip_neck_bn_gelu_bwd_sums(const void* da_bf16, const void* y_bf16, int64_t R, int D, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, float* workspace, size_t workspace_bytes, float* out,
                                 memhip_stream_t stream);
int memhip_neck_bn_gelu_bwd_apply(const void* da_bf16, const void* y_bf16, int64_t R, int D, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, const float* sums, float inv_n, void* dy_bf16,
                                  memhip_stream_t stream);

/* ------------------------------------------------------------------------
 * Segmentation loss and metrics (seg_loss.hip, seg_plan.cpp; additive to ABI 10)
 * replaces the end of every mmseg 0.30 decode head: resize(seg_logit, size=seg_label.shape[2:], mode='bilinear') ->
 *          cross_entropy(ignore_index=255) / accuracy (training) and resize -> argmax -> intersect_and_union (evaluation)
 *          mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-50
 * ------------------------------------------------------------------------
 * The upsampled [B, C, H, W] tensor is never written.  Both calls and the plan query read one host struct.
 *
 * Axis tables: the bilinear weights of one axis (in -> out samples, out >= in), torch's upsample_bilinear2d arithmetic in
 * fp32: scale = in / out (align_corners: (in - 1) / (out - 1), 0 when out == 1), src = max(scale (y + 0.5) - 0.5, 0)
 * (align_corners: scale y), i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), w1 = src - i0, w0 = 1 - w1.
 * lo[i] .. hi[i] is the inclusive range of outputs that read input i through i0 or i1.  memhip_seg_axis_table fills HOST
 * arrays i0[out], w1[out], lo[in], hi[in]; the caller uploads them and the kernels read the weights from there, so loss and
 * gradient agree on every weight.  A pixel's logit is w0y (w0x a + w1x b) + w1y (w0x c + w1x d). */
int memhip_seg_axis_table(int in, int out, int align_corners, int32_t* i0, float* w1, int32_t* lo, int32_t* hi);

/* (declared as a tagged struct with its typedef behind it, like memhip_seg_plan below) */
struct memhip_seg_args {
  const float* logits;               /* device f32, logical [B, C, h, w] at element strides sb, sc, sy, sx (NCHW of a torch
                                        head, or pixel rows [B h w, ld]: sb = h w ld, sc = 1, sy = w ld, sx = ld) */
  int64_t sb, sc, sy, sx;
  const uint8_t* labels;             /* device u8 [B, H, W] contiguous */
  int32_t B, C, h, w, H, W;          /* B >= 1, 2 <= C <= 32, H >= h >= 1, W >= w >= 1 */
  int32_t ignore_index;              /* the label that does not count (mmseg: 255); -1: none.  A label >= C that is not
                                        ignore_index is counted in n_bad and otherwise treated as ignored */
  int32_t align_corners;             /* 0 / 1 */
  int32_t avg_non_ignore;            /* 0: loss = loss_weight * sum / (B H W) (mmseg 0.30); 1: / max(n_valid, 1) */
  float loss_weight;
  const int32_t* y_i0; const float* y_w1; const int32_t* y_lo; const int32_t* y_hi;   /* device: the table (h -> H) */
  const int32_t* x_i0; const float* x_w1; const int32_t* x_lo; const int32_t* x_hi;   /* device: the table (w -> W) */
  /* memhip_seg_ce only */
  float* dz;                         /* device f32, logical [B, C, h, w] at element strides db, dc, dy, dx (no two elements
                                        at one address): sum over the outputs of weight * (softmax - onehot), UNSCALED;
                                        every element is written exactly once */
  int64_t db, dc, dy, dx;
  float* loss;                       /* device f32 [3]: loss, loss_weight / N (the factor of dz in the backward), loss_sum */
  int64_t* stats;                    /* device i64 [3]: n_valid, n_correct (argmax == label, ties to the lowest class), n_bad */
  void* workspace;                   /* device, workspace_bytes >= memhip_seg_plan_t.ws_bytes, 8-byte aligned */
  size_t workspace_bytes;
  /* memhip_seg_confusion only */
  int64_t* confusion;                /* device i64 [C, C], row = label, column = prediction: ADDED to */
};
typedef struct memhip_seg_args memhip_seg_args_t;

/* Training: one kernel (a workgroup per tile of low-resolution pixels recomputes the outputs in its footprint, takes loss and
 * counts of the outputs it is home to, gathers dz in a fixed order) + a one-workgroup finish kernel.  No float atomics:
 * the same inputs give the same bits.  All labels ignored: loss 0, dz 0. */
int memhip_seg_ce(const memhip_seg_args_t* args, memhip_stream_t stream);
/* Evaluation: one thread per output pixel, argmax of the interpolated logits (ties to the lowest class), a C x C histogram
 * per workgroup in LDS, flushed with integer atomics.  Ignored and bad labels are skipped. */
int memhip_seg_confusion(const memhip_seg_args_t* args, memhip_stream_t stream);

/* The launches of both calls as data.  memhip_seg_plan validates the struct like the calls do, except that pointers may
 * be NULL (workspace_bytes is compared only when there is a workspace).  Host arithmetic only. */
struct memhip_seg_plan {
  int32_t tile_h, tile_w;            /* low-resolution pixels per workgroup; tile (ty, tx) starts at (ty tile_h, tx tile_w) */
  int32_t tiles_y, tiles_x;
  int32_t grid, block;               /* memhip_seg_ce: grid = B tiles_y tiles_x workgroups, one workspace slot each */
  int32_t chunk;                     /* outputs of a footprint per pass */
  int32_t max_fh, max_fw;            /* the largest footprint (y_lo[first] .. y_hi[last] of a tile) over the tiles */
  int32_t tables_in_lds;             /* the footprint's slices of the tables are staged in LDS (else read from memory) */
  int32_t lds_bytes;                 /* per workgroup, <= 64 KiB */
  int32_t slot_bytes;                /* workspace bytes per workgroup */
  int32_t conf_grid, conf_block, conf_lds_bytes;   /* memhip_seg_confusion */
  int32_t reserved;
  uint64_t ws_bytes;
};
typedef struct memhip_seg_plan memhip_seg_plan_t;
int memhip_seg_plan(const memhip_seg_args_t* args, memhip_seg_plan_t* out);

/* ------------------------------------------------------------------------
 * Class weights and OHEM pixel sampling inside the fused loss (seg_ohem.hip, seg_loss.hip, seg_plan.cpp; additive to ABI 10)
 * replaces mmseg 0.30 CrossEntropyLoss(class_weight=...) and OHEMPixelSampler(thresh, min_kept)
 *          (mmseg/models/losses/cross_entropy_loss.py, mmseg/core/seg/sampler/ohem_pixel_sampler.py)
 * ------------------------------------------------------------------------
 * With z_p the resized logits of output pixel p (the tables above), l_p its label, valid as above, nll_p = logsumexp(z_p) -
 * z_p[l_p], cw the class weights (all ones when class_weight is NULL) and s_p in {0, 1} the sampler's pixel weight:
 *   loss = loss_weight / N * sum over valid p of cw[l_p] s_p nll_p,  N = B H W, or max(n_valid, 1) with avg_non_ignore
 *   dz   = sum over the outputs of weight * cw[l_p] s_p (softmax - onehot), UNSCALED as in memhip_seg_ce
 * N, n_valid, n_correct and n_bad depend on neither cw nor s (mmseg does not divide by the sum of the weights).
 *
 * The sampler is not differentiated through.  Its keys are fp32, computed once and stored as a [B, H, W] map; every keep
 * decision is taken on the stored keys, so the selection and the loss kernel cannot disagree about a pixel.  A key k counts
 * when k >= 0.0f (a NaN does not; -0.0f is 0.0f); memhip_seg_ohem_keys stores -1.0f at pixels that are not valid.  With n the
 * number of keys that count and K = min_kept * B:
 *   sampler 1 (thresh T):  key = softmax(z_p)[l_p].  n == 0: nothing kept.  Else, keys ascending a_0 <= .. <= a_n-1,
 *                          t = max(a_min(K, n-1), T) and s_p = [key_p < t].          *threshold = t;  -inf = keep none
 *   sampler 2 (top-k):     key = cw[l_p] nll_p.  K' = min(K, n); K' == 0: nothing kept.  Else, keys descending b_0 >= ..,
 *                          v = b_K'-1 and s_p = [key_p >= v].                        *threshold = v;  +inf = keep none
 *                          EVERY key equal to v is kept (mmseg keeps exactly K, by the order its sort leaves among ties).
 * "Keep all" has no value of its own: it is a t above every key (sampler 1), or v = the smallest key (sampler 2).
 * K is per process, as in mmseg: nothing is exchanged between ranks.
 *
 *   memhip_seg_ohem_keys:   logits, labels -> keys.  A thread per output pixel, max-subtracted softmax in fp32, the same
 *                           interpolation arithmetic as the loss kernel.  Reads class_weight with sampler 2.  The three calls
 *                           validate one struct alike: this call touches neither threshold nor the workspace, yet a NULL
 *                           threshold is rejected, and so is a workspace that is given and too small (NULL is fine).  A caller
 *                           that wants the key map alone passes any f32 [1] as threshold.
 *   memhip_seg_ohem_select: keys (which the caller may have written) -> *threshold and seg.stats[3] = n_kept, the number of
 *                           keys that count and pass the comparison.  An exact radix select on the keys' bit patterns
 *                           (non-negative floats order like their bits): three histogram passes over bits 31..21 / 20..10 / 9..0 (bit 31 is
 *                           zero in a key that counts, so the 31 value bits split 10 / 11 / 10 and the first pass fills 1024 of its bins), a
 *                           histogram per workgroup in LDS, nonzero bins flushed with 64-bit integer atomics, a
 *                           one-workgroup scan after each pass that finds the bin of rank r (n and r are derived on the device:
 *                           r = min(K, n - 1) ascending, or n - K'), then a counting pass.  No float atomics, no host read, no sort.
 *                           The call clears its part of the workspace on the stream before it counts: the caller prepares nothing.
 *   memhip_seg_ce_w:        memhip_seg_ce's kernel with q_c and the loss term multiplied by cw[l_p] s_p; cw is staged once per
 *                           workgroup, s_p is read from keys and *threshold; seg.stats is i64 [4]: n_valid, n_correct, n_bad,
 *                           n_kept (= n_valid without a sampler), counted at the pixel's home tile.  With class_weight NULL
 *                           and sampler 0, or with all weights 1.0f, loss, dz and stats[0..2] are memhip_seg_ce's bit for bit.
 * All three validate before any launch; memhip_seg_ohem_plan gives the same code and message, except that the device
 * pointers of seg may be NULL.  Rejected with MEMHIP_EINVAL: everything memhip_seg_plan rejects; a sampler other than 0, 1, 2;
 * with sampler 1 a thresh outside (0, 1]; with a sampler min_kept < 0 or > 2^40, or keys or threshold NULL; sampler 0 in
 * memhip_seg_ohem_keys / _select.  A workspace of fewer than ws_bytes bytes is MEMHIP_EWORKSPACE.  class_weight's entries must be
 * finite and >= 0: device memory, not read by the validation.
 * (Tagged structs with the typedef behind them; the tags say segohem, as memhip_segpredict_args says segpredict.) */
struct memhip_segohem_args {
  memhip_seg_args_t seg;             /* as for memhip_seg_ce; stats: device i64 [4]; workspace_bytes >= memhip_segohem_plan_t.ws_bytes;
                                        confusion is not read */
  const float* class_weight;         /* device f32 [C], or NULL: all ones */
  int32_t sampler;                   /* 0 none, 1 thresh, 2 top-k */
  float thresh;                      /* T, sampler 1 */
  int64_t min_kept;                  /* m */
  float* keys;                       /* device f32 [B, H, W], caller-provided */
  float* threshold;                  /* device f32 [1]: t or v */
};
typedef struct memhip_segohem_args memhip_segohem_args_t;
int memhip_seg_ohem_keys(const memhip_segohem_args_t* args, memhip_stream_t stream);
int memhip_seg_ohem_select(const memhip_segohem_args_t* args, memhip_stream_t stream);
int memhip_seg_ce_w(const memhip_segohem_args_t* args, memhip_stream_t stream);

/* The launches of the three calls as data.  Host arithmetic only. */
struct memhip_segohem_plan {
  memhip_seg_plan_t seg;             /* memhip_seg_ce_w's kernel: memhip_seg_ce's plan, lds_bytes with the staged class weights */
  int32_t keys_grid, keys_block;     /* memhip_seg_ohem_keys: strides over the pixels beyond keys_grid workgroups */
  int32_t select_grid, select_block; /* the histogram and counting passes of memhip_seg_ohem_select */
  int32_t select_passes, select_bins;/* 3 passes, 2048 bins (the last pass uses 1024) */
  int32_t select_lds_bytes;          /* a workgroup's histogram */
  int32_t reserved;
  uint64_t select_ws_offset;         /* the selection's part of the workspace: [offset, offset + bytes), cleared by the call */
  uint64_t select_ws_bytes;          /* 0 without a sampler */
  uint64_t ws_bytes;                 /* seg.ws_bytes (the partials, rounded up to 8) + select_ws_bytes */
};
typedef struct memhip_segohem_plan memhip_segohem_plan_t;
int memhip_seg_ohem_plan(const memhip_segohem_args_t* args, memhip_segohem_plan_t* out);

/* ------------------------------------------------------------------------
 * Segmentation inference: logits of V views -> label map (seg_predict.hip, seg_predict_plan.cpp; additive to ABI 10)
 * replaces mmseg 0.30 EncoderDecoder.slide_inference / whole_inference / inference / aug_test behind encode_decode
 *          (mmseg/models/segmentors/encoder_decoder.py), reached from
 *          mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:53 (test_cfg) and
 *          mem/semantic_segmentation/tools/test.py:94-99 (single_gpu_test / multi_gpu_test)
 * ------------------------------------------------------------------------
 * A view is one run of the model on one window of one flip state of the canvas [H, W].  All views share the window size
 * (hc, wc) and the logits size (h, w), and with them one pair of axis tables (h -> hc, w -> wc) of memhip_seg_axis_table,
 * of which i0 and w1 are read.  One gather kernel, a thread per four consecutive output pixels of a row; no upsampled tensor
 * and no per-window canvas is written.  rects is a HOST array i32 [V, 3] = {y1, x1, flip}, copied into the kernel's
 * arguments; with flip = 1 the rectangle is in the coordinates of the horizontally flipped canvas.
 *
 * For pass f among the flip values present (one or two passes):
 *   L_f(y, x, c) = sum over the views of pass f whose rectangle holds (y, x), in the order of rects, of the bilinear logit at
 *                  (y - y1, x - x1) -- w0y (w0x a + w1x b) + w1y (w0x c + w1x d) in fp32 -- divided by their number
 *                  (slide_inference: preds += F.pad(crop_seg_logit, ...); count_mat += 1; preds / count_mat)
 *   P_f = softmax_c(L_f), the maximum subtracted                                       (inference: F.softmax(seg_logit, dim=1))
 *   output pixel (y, x) reads pass 1 at (y, W - 1 - x)                                 (inference: output.flip(dims=(3,)))
 *   P = mean of P_f over the passes; pred = argmax_c P, ties to the lowest class       (aug_test: seg_logit /= len(imgs))
 * With one pass the argmax is taken on L_f itself (softmax keeps an argmax), so one view that covers the canvas gives the
 * labels of memhip_seg_confusion bit for bit.  Whole-image mode is V = 1, rectangle (0, 0), (hc, wc) = (H, W).
 *
 * Outputs, each optional (NULL = off), at least one: pred u8 [B, H, W]; prob f32 [B, C, H, W] = P; labels u8 [B, H, W] with
 * confusion i64 [C, C] (row = label, column = pred; ADDED to; labels equal to ignore_index or >= C are skipped, as in
 * memhip_seg_confusion; both set or both NULL).  The histogram of a workgroup lives in LDS and is flushed with 64-bit integer
 * atomics.  No float atomics: two calls give the same bits.  No host synchronisation, no allocation, nothing is written
 * outside the outputs.
 *
 * Rejected with MEMHIP_EINVAL before any launch, by the call and by the plan query alike: V outside 1 .. 64; C outside
 * 2 .. 32; hc < h, wc < w, h < 1, w < 1; hc > H, wc > W; a rectangle that leaves the canvas; a flip value other than 0 / 1;
 * a pass in which a pixel of the canvas is covered by no view (host arithmetic over the rectangles); labels without confusion
 * or the reverse; no output.  B == 0 is MEMHIP_OK, nothing is read.  Not carried: vertical flips, multi-scale views (views
 * of different sizes), more than 64 views per call.
 * (Tagged structs with the typedef behind them, like memhip_seg_args; the tags say segpredict, as memhip_segdata_args says
 * segdata: the `struct memhip_seg_*` of this header are the loss's two.) */
struct memhip_segpredict_args {
  const float* logits;               /* device f32, logical [V, B, C, h, w] at element strides sv, sb, sc, sy, sx (the views
                                        stacked in the batch of the model call: sv = B sb; NCHW, or the heads' pixel rows
                                        [V B h w, ld]: sb = h w ld, sc = 1, sy = w ld, sx = ld) */
  int64_t sv, sb, sc, sy, sx;
  const int32_t* rects;              /* HOST i32 [V, 3] = {y1, x1, flip}, read during the call */
  int32_t V, B, C, h, w;             /* 1 <= V <= 64, 2 <= C <= 32, h, w >= 1 */
  int32_t hc, wc;                    /* the window: hc >= h, wc >= w */
  int32_t H, W;                      /* the canvas: H >= hc, W >= wc */
  int32_t align_corners;             /* 0 / 1: what the tables were made with */
  int32_t ignore_index;              /* labels: the value that does not count (mmseg: 255); -1: none */
  int32_t reserved0;
  const int32_t* y_i0; const float* y_w1;   /* device: the table (h -> hc) */
  const int32_t* x_i0; const float* x_w1;   /* device: the table (w -> wc) */
  uint8_t* pred;                     /* device u8 [B, H, W] or NULL */
  float* prob;                       /* device f32 [B, C, H, W] or NULL */
  const uint8_t* labels;             /* device u8 [B, H, W] or NULL */
  int64_t* confusion;                /* device i64 [C, C] or NULL: ADDED to */
};
typedef struct memhip_segpredict_args memhip_segpredict_args_t;
int memhip_seg_predict(const memhip_segpredict_args_t* args, memhip_stream_t stream);

/* The launch as data.  memhip_seg_predict_plan validates the struct like the call does, except that the device pointers of
 * logits and tables may be NULL (rects is host memory and is read).  Host arithmetic only. */
struct memhip_segpredict_plan {
  int32_t tile_h, tile_w;            /* output pixels per workgroup; tile (ty, tx) starts at (ty tile_h, tx tile_w) */
  int32_t tiles_y, tiles_x;
  int32_t grid, block;               /* grid = B tiles_y tiles_x */
  int32_t lds_bytes;                 /* the workgroup's histogram */
  int32_t pixels_per_thread;         /* consecutive x of one row */
  int32_t padded_classes;            /* the instantiation: 8, 12, .. 32 */
  int32_t passes;                    /* 1 or 2: the flip values present */
  int32_t max_count;                 /* the largest number of views of one pass that cover one pixel */
  int32_t pred_dwords;               /* pred leaves as whole dwords (W a multiple of 4 and pred 4-byte aligned) */
};
typedef struct memhip_segpredict_plan memhip_segpredict_plan_t;
int memhip_seg_predict_plan(const memhip_segpredict_args_t* args, memhip_segpredict_plan_t* out);

/* ------------------------------------------------------------------------
 * FCN decode head (seg_head.hip, seg_head_plan.cpp; additive to ABI 10)
 * replaces auxiliary_head = dict(type='FCNHead', in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1,
 *          norm_cfg=SyncBN, align_corners=False)   mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:38-50
 *                                                  mem/semantic_segmentation/configs/mem/upernet/mem_224_160k.py:64-77
 *          mmseg 0.30 FCNHead.forward: output = self.convs(x) [ConvModule: Conv2d(3, padding 1, bias=False) -> SyncBN -> ReLU];
 *          BaseDecodeHead.cls_seg: self.conv_seg(self.dropout(feat)) [Dropout2d -> Conv2d(channels, num_classes, 1)]
 * ------------------------------------------------------------------------
 * The 3x3 convolution, its data gradient and its weight gradient are memhip_conv2d_nhwc (MEMHIP_CONV_BF16) and
 * memhip_conv_wgrad_nhwc on the activation format of the tokenizer: bf16 [B, h+2, w+2, C], a one-pixel zero border.  What
 * is declared here is everything around them; every kernel streams, 16 bytes per lane, no float atomics (two calls give the
 * same bits), nothing reads the environment.  B == 0 is MEMHIP_OK everywhere, nothing is read.
 *
 * Movers between the engine's fp32 maps and that format, through a padded 64 x 64 LDS tile like memhip_tokens_to_maps:
 * memhip_map_to_nhwc_pad: map f32 [B, D, h, w] -> the INTERIOR of out bf16 [B, h+2, w+2, D] (round to nearest even; the
 *   ring is never written: the caller zeroes the buffer once).  memhip_nhwc_pad_to_map: the inverse, bf16 -> f32 (exact).
 * D % 64 == 0, any h, w >= 1 (ragged tiles are neither read nor written); the bf16 buffer 16-byte aligned; the map side
 * moves 16 bytes per lane when h w % 4 == 0 and the map is 16-byte aligned, single floats otherwise. */
int memhip_map_to_nhwc_pad(const float* map, int B, int D, int h, int w, void* out_bf16, memhip_stream_t stream);
int memhip_nhwc_pad_to_map(const void* in_bf16, int B, int D, int h, int w, float* map, memhip_stream_t stream);
/* Batch statistics of a bf16 activation of C channels (C % 64 == 0) over its R = B h w pixels: padded = 1: the
 * one-pixel-border format [B, h+2, w+2, C], only interiors are read; 0: dense rows [R, C].  shift f32 [C] or NULL (zero).
 *   out f32 [3, C] = count (R), sum (x - shift), sum (x - shift)^2 per channel
 * Two stages: G = min(ceil(R / 32), MEMHIP_BN_GROUPS) workgroups per 64 channels, each thread a fixed-order chain over its
 * rows r = 32 g + j, + 32 G, .., the 32 row lanes folded in LDS in order, one partial per workgroup stored plainly to
 * `workspace` (memhip_bn_stats_workspace(C) bytes), and a finish kernel that adds the G partials in order.  The longest
 * chain of fp32 roundings behind one output (the subtraction and the square included) is ceil(R / (32 G)) + 32 + G. */
#define MEMHIP_BN_GROUPS 128
size_t memhip_bn_stats_workspace(int C);
int memhip_bn_stats_nhwc(const void* x_bf16, int padded, int B, int h, int w, int C, const float* shift, float* workspace,
                         size_t workspace_bytes, float* out, memhip_stream_t stream);

/* The site of memhip_dropout_t's mask contract for decode heads: Dropout2d drops a whole channel of a sample, element
 * (site = MEMHIP_DROPOUT_SITE_HEAD + head number, row = sample b, col = channel c), so that
 * memhip_dropout_mask(d, 0, B, C) reproduces the bits.  The trunk's sites are 0 .. 2 depth; this constant is above 2 depth
 * for any depth (a depth is far below 2^30). */
#define MEMHIP_DROPOUT_SITE_HEAD 0x48454144u

/* The fused tail of the head over the convolution's output y (bf16 padded, C channels; C % 64 == 0, C <= 512) and the 1x1
 * classifier wcls f32 [K, C], 2 <= K <= 32 (the segmentation loss's limit).  With xhat = (y - mean) rstd,
 * u = gamma xhat + beta, keep = the Dropout2d bit of (sample, channel) and scale = 1 / (1 - p) (dropout NULL: 1, 1), all fp32:
 *   memhip_bnhead_fwd:       z = relu(u) keep scale (not stored); logits[r, k] = bias[k] + sum_c z[c] wcls[k, c] as f32 pixel
 *                            rows [R, ld], ld >= K: memhip_seg_args_t's layout with sb = h w ld, sc = 1, sy = w ld, sx = ld.
 *                            The classifier weight is staged in LDS once per workgroup (K C 4 <= 64 KiB).
 *   memhip_bnhead_bwd_sums:  from dlogit f32, logical [B, K, h, w] at element strides db, dk, dy, dx (memhip_seg_args_t.dz as
 *                            it is), dz[c] = sum_k dlogit[k] wcls[k, c], g = dz keep scale (u > 0):
 *                            sums f32 [2, C] = sum g (= dbeta), sum g xhat (= dgamma); dwcls f32 [K, C] = sum_pixels dlogit[k] z[c];
 *                            dbias f32 [K] = sum_pixels dlogit[k].  Per-workgroup partials as plain stores into `workspace`
 *                            (memhip_bnhead_plan_t.ws_bytes), folded in ascending order by a second launch; all four overwritten.
 *   memhip_bnhead_bwd_apply: dy bf16 = gamma rstd (g - tot[0, c] inv_n - xhat tot[1, c] inv_n) into the INTERIOR of the padded
 *                            format (the ring is never written), where the dgrad convolution reads it and
 *                            memhip_conv_wgrad_nhwc takes it as small_padded = 1.  tot f32 [2, C] = the (all-reduced) sums and
 *                            inv_n = 1 / (elements per channel over all ranks) are arguments, so that a SyncBN exchange sits
 *                            between the two calls; tot NULL: eval statistics (running stats, a frozen BN), no correction terms.
 * mean / rstd / gamma / beta f32 [C]; they, wcls, y and dy 16-byte aligned.  A field another call owns is ignored.
 * (The structs are declared tag first, typedef second.) */
struct memhip_bnhead_args {
  const void* y;                     /* device bf16 [B, h+2, w+2, C] */
  const float* mean; const float* rstd; const float* gamma; const float* beta;   /* device f32 [C] */
  const float* wcls;                 /* device f32 [K, C] */
  const float* bias;                 /* device f32 [K], or NULL (memhip_bnhead_fwd only) */
  const memhip_dropout_t* dropout;   /* HOST struct read at the call, or NULL: nothing dropped */
  int32_t B, C, K, h, w;
  int32_t reserved0;
  /* memhip_bnhead_fwd */
  float* logits;                     /* device f32 [B h w, ld] */
  int64_t ld;                        /* >= K (the plan query: 0 = not given) */
  /* memhip_bnhead_bwd_sums and _apply */
  const float* dlogit;               /* device f32, logical [B, K, h, w] at element strides db, dk, dy, dx */
  int64_t db, dk, dy, dx;
  /* memhip_bnhead_bwd_sums */
  float* sums;                       /* device f32 [2, C] */
  float* dwcls;                      /* device f32 [K, C] */
  float* dbias;                      /* device f32 [K] */
  void* workspace;                   /* device, workspace_bytes >= memhip_bnhead_plan_t.ws_bytes, 16-byte aligned */
  size_t workspace_bytes;
  /* memhip_bnhead_bwd_apply */
  const float* tot;                  /* device f32 [2, C], or NULL: eval statistics */
  float inv_n;                       /* > 0 when tot is given */
  int32_t reserved1;
  void* dy_out;                      /* device bf16 [B, h+2, w+2, C] */
};
typedef struct memhip_bnhead_args memhip_bnhead_args_t;
int memhip_bnhead_fwd(const memhip_bnhead_args_t* args, memhip_stream_t stream);
int memhip_bnhead_bwd_sums(const memhip_bnhead_args_t* args, memhip_stream_t stream);
int memhip_bnhead_bwd_apply(const memhip_bnhead_args_t* args, memhip_stream_t stream);

/* The launches of the three calls as data.  memhip_bnhead_plan validates the struct like the calls do (same codes and
 * messages), except that pointers may be NULL (workspace_bytes is compared only when there is a workspace; ld only when it
 * is not 0).  Host arithmetic only. */
struct memhip_bnhead_plan {
  int64_t R;                         /* B h w pixels (0: nothing to do) */
  int32_t kp;                        /* classifier rows held per thread: K rounded up to a multiple of 8 */
  int32_t block;                     /* threads of every launch */
  int32_t fwd_grid, fwd_lds_bytes;   /* tiles of 32 pixels, strided over by at most 512 workgroups; the weight [kp, C] */
  int32_t sums_grid_x, sums_grid_y, sums_lds_bytes;   /* x: pixel groups (tiles of 64 pixels, at most MEMHIP_BN_GROUPS), y: C / 64 */
  int32_t apply_grid_x, apply_grid_y, apply_lds_bytes;   /* x: tiles of 32 pixels, y: C / 64 */
  int32_t slot_floats;               /* workspace floats per pixel group: 2 C + K C + K */
  int32_t fold_grid;                 /* workgroups of the fold launch */
  uint64_t ws_bytes;
};
typedef struct memhip_bnhead_plan memhip_bnhead_plan_t;
int memhip_bnhead_plan(const memhip_bnhead_args_t* args, memhip_bnhead_plan_t* out);

/* ------------------------------------------------------------------------
 * Pyramid pooling of the PSP decode head (ppm.hip, ppm_plan.cpp; additive to ABI 10)
 * replaces mmseg 0.30 PSPHead.forward / UPerHead.psp_forward up to the bottleneck's operand
 *          (mmseg/models/decode_heads/psp_head.py: PPM = per pool scale AdaptiveAvgPool2d(s) -> ConvModule(1x1, no bias,
 *          SyncBN, ReLU) -> resize(bilinear, size of the input); psp_outs = cat([x] + ppm_outs, dim=1) -> bottleneck)
 *          decode_head = dict(type='UPerHead', pool_scales=(1, 2, 3, 6), channels=512, ...)
 *          mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37
 * ------------------------------------------------------------------------
 * Everything is on the activation format of the FCN head above: bf16 [B, m+2, m'+2, channels] with a zero ring that is never
 * written.  n <= MEMHIP_PPM_MAX_SCALES pool scales, 1 <= s <= MEMHIP_PPM_MAX_SCALE, s <= min(h, w).  Per scale i:
 *   P_i  bf16 [B, s+2, s+2, Cin]  the pooled map, operand of the 1x1 convolution (memhip_conv2d_nhwc) and of its weight gradient
 *   Y_i  bf16 [B, s+2, s+2, C]    the 1x1 convolution's output; its batch statistics are memhip_bn_stats_nhwc
 * and Xcat bf16 [B, h+2, w+2, Cin + n C] is the operand of the bottleneck's 3x3 convolution: channels [0, Cin) the map,
 * channels Cin + i C + c the upsampled activation of scale i.  Neither relu(bn(Y_i)) nor an upsampled map nor an fp32 concat
 * is ever stored.  mean / rstd / gamma / beta / sums / tot are f32 [n, C] resp. [n, 2, C], scale-major.
 *
 * Pool bins: bin i of s over n pixels is [floor(i n / s), ceil((i + 1) n / s)), integer arithmetic; memhip_ppm_bins fills
 * HOST arrays start[s], end[s] with the arithmetic the kernels use.  With s <= n a pixel lies in at most two bins per axis.
 * Bilinear weights: memhip_seg_axis_table(s, h, ...) and (s, w, ...) of the segmentation loss, uploaded by the caller; forward
 * and backward read the same tables.  Taps combine as w0y (w0x a + w1x b) + w1y (w0x c + w1x d).
 *
 *   memhip_ppm_pool:             map f32 [B, Cin, h, w], read once -> the interiors of all P_i in one launch: the fp32 sum of a
 *                                bin in row-major order, divided by the bin's pixel count, rounded to bf16 (nearest even).  A
 *                                bin of one pixel holds the bits of memhip_map_to_nhwc_pad.
 *   memhip_ppm_concat_fwd:       the interior of Xcat in one launch: channels [0, Cin) the bits of memhip_map_to_nhwc_pad; channel
 *                                Cin + i C + c = bf16(bilinear(relu(gamma xhat + beta))), xhat = (Y_i - mean) rstd at the four taps.
 *   memhip_ppm_concat_bwd_sums:  from dXcat (channels >= Cin): dA[b, bin, c] = the sum over the outputs lo .. hi of both axes
 *                                of (wy wx) dXcat, rows then columns ascending; g_i f32 [B s^2, C] = dA (u > 0); sums f32
 *                                [n, 2, C] = sum g, sum g xhat over (b, bin): 32 row lanes, each an ascending chain, folded in
 *                                order by the one workgroup that owns the 64 channels.
 *   memhip_ppm_bwd_apply:        the interiors of dY_i bf16 = gamma rstd (g - tot[i, 0] inv_n[i] - xhat tot[i, 1] inv_n[i]);
 *                                tot NULL: eval statistics, no correction terms.
 *   memhip_ppm_dmap:             dmap f32 [B, Cin, h, w], overwritten = f32(dXcat[.., c < Cin]) + for each scale, bin row and bin
 *                                column holding the pixel (in that order, at most 2 x 2 per scale) f32(dP_i) / count(bin).
 * No float atomics, no workspace: every sum is a gather in an order fixed by the shapes alone, so two calls give the same
 * bits.  Every bf16 buffer and vector 16-byte aligned.  One host struct for the five calls and the plan; a field another call
 * owns is ignored.  B == 0 is MEMHIP_OK, nothing is read. */
#define MEMHIP_PPM_MAX_SCALES 4
#define MEMHIP_PPM_MAX_SCALE 8
int memhip_ppm_bins(int n, int s, int32_t* start, int32_t* end);

struct memhip_ppm_args {
  int32_t B, Cin, C, h, w;
  int32_t n;                         /* pool scales, 1 .. MEMHIP_PPM_MAX_SCALES */
  int32_t scales[MEMHIP_PPM_MAX_SCALES];
  const float* map;                  /* device f32 [B, Cin, h, w] (_pool, _concat_fwd) */
  void* P[MEMHIP_PPM_MAX_SCALES];    /* device bf16 [B, s+2, s+2, Cin] (_pool writes the interiors) */
  const void* Y[MEMHIP_PPM_MAX_SCALES];   /* device bf16 [B, s+2, s+2, C] (_concat_fwd, _concat_bwd_sums, _bwd_apply) */
  const float* mean; const float* rstd; const float* gamma; const float* beta;   /* device f32 [n, C] */
  /* device: the tables (s -> h) and (s -> w) of memhip_seg_axis_table per scale (_concat_fwd, _concat_bwd_sums) */
  const int32_t* y_i0[MEMHIP_PPM_MAX_SCALES]; const float* y_w1[MEMHIP_PPM_MAX_SCALES];
  const int32_t* y_lo[MEMHIP_PPM_MAX_SCALES]; const int32_t* y_hi[MEMHIP_PPM_MAX_SCALES];
  const int32_t* x_i0[MEMHIP_PPM_MAX_SCALES]; const float* x_w1[MEMHIP_PPM_MAX_SCALES];
  const int32_t* x_lo[MEMHIP_PPM_MAX_SCALES]; const int32_t* x_hi[MEMHIP_PPM_MAX_SCALES];
  void* xcat;                        /* device bf16 [B, h+2, w+2, Cin + n C] (_concat_fwd writes the interior) */
  const void* dxcat;                 /* device bf16, the same shape (_concat_bwd_sums: channels >= Cin, _dmap: channels < Cin) */
  float* g[MEMHIP_PPM_MAX_SCALES];   /* device f32 [B s^2, C] (_concat_bwd_sums writes, _bwd_apply reads) */
  float* sums;                       /* device f32 [n, 2, C] (_concat_bwd_sums) */
  const float* tot;                  /* device f32 [n, 2, C], or NULL: eval statistics (_bwd_apply) */
  float inv_n[MEMHIP_PPM_MAX_SCALES];     /* > 0 when tot is given */
  void* dY[MEMHIP_PPM_MAX_SCALES];   /* device bf16 [B, s+2, s+2, C] (_bwd_apply writes the interiors) */
  const void* dP[MEMHIP_PPM_MAX_SCALES];  /* device bf16 [B, s+2, s+2, Cin] (_dmap) */
  float* dmap;                       /* device f32 [B, Cin, h, w] (_dmap) */
};
typedef struct memhip_ppm_args memhip_ppm_args_t;
int memhip_ppm_pool(const memhip_ppm_args_t* args, memhip_stream_t stream);
int memhip_ppm_concat_fwd(const memhip_ppm_args_t* args, memhip_stream_t stream);
int memhip_ppm_concat_bwd_sums(const memhip_ppm_args_t* args, memhip_stream_t stream);
int memhip_ppm_bwd_apply(const memhip_ppm_args_t* args, memhip_stream_t stream);
int memhip_ppm_dmap(const memhip_ppm_args_t* args, memhip_stream_t stream);

/* The launches of the five calls as data.  memhip_ppm_plan validates the struct like the calls do (same codes and messages),
 * except that pointers may be NULL.  Host arithmetic only. */
struct memhip_ppm_plan {
  int64_t R;                         /* B h w pixels (0: nothing to do) */
  int32_t block;                     /* threads of every launch */
  int32_t ct;                        /* channels of Xcat: Cin + n C */
  int32_t bins;                      /* sum of s^2 */
  int32_t rows[MEMHIP_PPM_MAX_SCALES];        /* B s^2 */
  int32_t row_tile0[MEMHIP_PPM_MAX_SCALES];   /* the first tile of 32 rows of scale i in the (scale, row) grids */
  int32_t pool_grid, pool_lds_bytes;          /* a workgroup per (sample, 64 channels): the tile and the bins' accumulators */
  int32_t concat_grid_x, concat_grid_y;       /* x: tiles of 64 pixels, y: Cin / 64 map tiles, then n C / 64 pyramid tiles */
  int32_t gather_grid_x, gather_grid_y;       /* _concat_bwd_sums, first launch, and _bwd_apply: x: tiles of 32 rows over the
                                                 scales, y: C / 64 */
  int32_t sums_grid_x, sums_grid_y;           /* _concat_bwd_sums, second launch: x: n, y: C / 64 */
  int32_t dmap_grid_x, dmap_grid_y;           /* x: tiles of 64 pixels, y: Cin / 64 */
  int32_t tile_lds_bytes;                     /* the 64 x 64 fp32 tile of _concat_fwd and _dmap; the fold's scratch of the sums */
  uint64_t ws_bytes;                          /* 0: no call takes a workspace */
};
typedef struct memhip_ppm_plan memhip_ppm_plan_t;
int memhip_ppm_plan(const memhip_ppm_args_t* args, memhip_ppm_plan_t* out);

/* ------------------------------------------------------------------------
 * The FPN part of the UPerNet decode head (fpn.hip, fpn_plan.cpp; additive to ABI 10)
 * replaces mmseg 0.30 UPerHead.forward between the convolutions (mmseg/models/decode_heads/uper_head.py): the top-down
 *          path laterals[i - 1] += resize(laterals[i], size of i - 1, bilinear), and fpn_outs[i] = resize(fpn_outs[i], size
 *          of level 0); cat(fpn_outs, dim=1) -> fpn_bottleneck; every ConvModule Conv2d(no bias) -> SyncBN -> ReLU
 *          decode_head = dict(type='UPerHead', in_index=[0, 1, 2, 3], channels=512, ...)
 *          mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37
 * ------------------------------------------------------------------------
 * L levels (2 .. MEMHIP_FPN_MAX_LEVELS) of h[l] x w[l] pixels, finest first, non-increasing in both axes (the tables resize
 * upwards only; equal sizes are allowed), all of C channels (C % 64 == 0, C <= 512).  Everything is on the activation format
 * of the heads above: bf16 [B, h_l+2, w_l+2, channels] with a ring that is neither read nor written.  The 1x1 / 3x3
 * convolutions, their data and weight gradients and the batch statistics are memhip_conv2d_nhwc / memhip_conv_wgrad_nhwc /
 * memhip_bn_stats_nhwc.  Per level l:
 *   Y[l]   bf16  a stored convolution output whose ReLU(SyncBN(.)) a call evaluates on the fly: which one is the caller's
 *                business (the lateral's, the FPN convolution's, at l = L - 1 the pyramid bottleneck's "Ypsp")
 *   T_l    bf16  the top-down sum, operand of FPN convolution l
 * BN vectors mean / rstd / gamma / beta are f32 [L, C], level-major: row l belongs to Y[l].
 * Bilinear weights: memhip_seg_axis_table(n_in, n_out, ...) uploaded by the caller, two families: "c" (h_l -> h_0, w_l ->
 * w_0: the concat) and "t" (h_{l+1} -> h_l, w_{l+1} -> w_l, stored at index l: the top-down step).  Forward and backward read
 * the same tables; taps combine as w0y (w0x a + w1x b) + w1y (w0x c + w1x d), u = gamma xhat + beta with xhat = (Y - mean) rstd.
 *
 *   memhip_fpn_topdown_fwd:  level = l <= L - 2.  The interior of T (= T_l) = bf16(relu(u(Y[l])) + bilinear_{l+1 -> l}(src)),
 *                            src = the stored T_{l+1} (`src`, plain bf16), or with src NULL (l == L - 2 only) relu(u(Y[l+1]))
 *                            evaluated in fp32 at the four taps: the activated coarsest lateral is never stored.
 *   memhip_fpn_concat_fwd:   the interior of xcat bf16 [B, h_0+2, w_0+2, L C] in one launch: channel l C + c =
 *                            bf16(bilinear_{l -> 0}(relu(u(Y[l])))).  An identity table (every w1 == 0, level 0 always)
 *                            gives exactly bf16(relu(u(Y[l]))).
 *   memhip_fpn_resize_bwd:   level = the destination d.  rows f32 [B h_d w_d, C] = the sum, in this order, of
 *                            own (bf16 padded map of the destination's size, or NULL), the transposed resize of channel
 *                            slice `slice` of dxcat (bf16, pitch L C, table c[d]; or NULL) and the transposed resize of
 *                            fine_rows f32 [B h_{d-1} w_{d-1}, C] (table t[d-1]; or NULL; d >= 1).  A transposed resize is
 *                            a gather over the outputs lo .. hi of both axes, rows then columns ascending, one fused
 *                            multiply-add each.  The rows are ungated.
 *   memhip_fpn_bn_bwd_sums:  level = l.  sums f32 [2, C] = sum g, sum g xhat over the B h_l w_l pixels, g = rows (u(Y[l]) > 0).
 *                            Two stages as memhip_bn_stats_nhwc: G = min(ceil(R / 32), MEMHIP_BN_GROUPS) workgroups per 64
 *                            channels, a fixed-order chain per thread over the rows r = 32 g + j, + 32 G, .., the 32 row
 *                            lanes folded in LDS in order, one partial per workgroup stored plainly into `workspace`
 *                            (memhip_fpn_plan_t.ws_bytes), the G partials added in ascending order by a second launch.
 *   memhip_fpn_bn_bwd_apply: level = l.  The interior of dY bf16 = gamma rstd (g - tot[0] inv_n - xhat tot[1] inv_n), g as
 *                            above; tot f32 [2, C], or NULL: eval statistics, no correction terms.
 * No float atomics: two calls give the same bits.  Every bf16 buffer, vector and f32 row buffer 16-byte aligned.  One host
 * struct for the five calls and the plan; NULL / 0 = off; a field another call owns is ignored.  B == 0 is MEMHIP_OK, nothing
 * is read. */
#define MEMHIP_FPN_MAX_LEVELS 4

struct memhip_fpn_args {
  int32_t B, C, L;
  int32_t level;                     /* 0 .. L - 1: the level of a per-level call (every call but _concat_fwd) */
  int32_t h[MEMHIP_FPN_MAX_LEVELS];
  int32_t w[MEMHIP_FPN_MAX_LEVELS];
  const void* Y[MEMHIP_FPN_MAX_LEVELS];   /* device bf16 [B, h_l+2, w_l+2, C] */
  const float* mean; const float* rstd; const float* gamma; const float* beta;   /* device f32 [L, C] */
  /* device: the tables (h_l -> h_0) and (w_l -> w_0) per level (_concat_fwd: all; _resize_bwd: of `level`, with dxcat) */
  const int32_t* cy_i0[MEMHIP_FPN_MAX_LEVELS]; const float* cy_w1[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* cy_lo[MEMHIP_FPN_MAX_LEVELS]; const int32_t* cy_hi[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* cx_i0[MEMHIP_FPN_MAX_LEVELS]; const float* cx_w1[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* cx_lo[MEMHIP_FPN_MAX_LEVELS]; const int32_t* cx_hi[MEMHIP_FPN_MAX_LEVELS];
  /* device: the tables (h_{l+1} -> h_l) and (w_{l+1} -> w_l) at index l (_topdown_fwd: of `level`; _resize_bwd: of
     `level` - 1, with fine_rows) */
  const int32_t* ty_i0[MEMHIP_FPN_MAX_LEVELS]; const float* ty_w1[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* ty_lo[MEMHIP_FPN_MAX_LEVELS]; const int32_t* ty_hi[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* tx_i0[MEMHIP_FPN_MAX_LEVELS]; const float* tx_w1[MEMHIP_FPN_MAX_LEVELS];
  const int32_t* tx_lo[MEMHIP_FPN_MAX_LEVELS]; const int32_t* tx_hi[MEMHIP_FPN_MAX_LEVELS];
  /* memhip_fpn_topdown_fwd */
  const void* src;                   /* device bf16 [B, h_{l+1}+2, w_{l+1}+2, C]: T_{l+1}; NULL: relu(u(Y[l+1])), l == L - 2 */
  void* T;                           /* device bf16 [B, h_l+2, w_l+2, C] */
  /* memhip_fpn_concat_fwd */
  void* xcat;                        /* device bf16 [B, h_0+2, w_0+2, L C] */
  /* memhip_fpn_resize_bwd */
  const void* own;                   /* device bf16 [B, h_d+2, w_d+2, C], or NULL */
  const void* dxcat;                 /* device bf16 [B, h_0+2, w_0+2, L C], or NULL */
  const float* fine_rows;            /* device f32 [B h_{d-1} w_{d-1}, C], or NULL */
  int32_t slice;                     /* 0 .. L - 1: the channel slice of dxcat */
  int32_t reserved0;
  float* rows;                       /* device f32 [B h_d w_d, C]: _resize_bwd writes, _bn_bwd_sums and _bn_bwd_apply read */
  /* memhip_fpn_bn_bwd_sums */
  float* sums;                       /* device f32 [2, C] */
  void* workspace;                   /* device, workspace_bytes >= memhip_fpn_plan_t.ws_bytes, 16-byte aligned */
  size_t workspace_bytes;
  /* memhip_fpn_bn_bwd_apply */
  const float* tot;                  /* device f32 [2, C], or NULL: eval statistics */
  float inv_n;                       /* > 0 when tot is given */
  int32_t reserved1;
  void* dY;                          /* device bf16 [B, h_l+2, w_l+2, C] */
};
typedef struct memhip_fpn_args memhip_fpn_args_t;
int memhip_fpn_topdown_fwd(const memhip_fpn_args_t* args, memhip_stream_t stream);
int memhip_fpn_concat_fwd(const memhip_fpn_args_t* args, memhip_stream_t stream);
int memhip_fpn_resize_bwd(const memhip_fpn_args_t* args, memhip_stream_t stream);
int memhip_fpn_bn_bwd_sums(const memhip_fpn_args_t* args, memhip_stream_t stream);
int memhip_fpn_bn_bwd_apply(const memhip_fpn_args_t* args, memhip_stream_t stream);

/* The launches of the five calls as data, for every level at once.  memhip_fpn_plan validates the struct like the calls do
 * (same codes and messages), except that pointers may be NULL (workspace_bytes is compared only when there is a workspace).
 * Host arithmetic only. */
struct memhip_fpn_plan {
  int64_t R[MEMHIP_FPN_MAX_LEVELS];           /* B h_l w_l pixels (0: nothing to do) */
  int32_t block;                              /* threads of every launch */
  int32_t ct;                                 /* channels of xcat: L C */
  int32_t grid_y;                             /* C / 64: every per-level launch */
  int32_t concat_grid_x, concat_grid_y;       /* x: tiles of 64 pixels of level 0, y: L C / 64 */
  int32_t topdown_grid_x[MEMHIP_FPN_MAX_LEVELS];   /* tiles of 64 pixels of level l (0 at l = L - 1) */
  int32_t resize_grid_x[MEMHIP_FPN_MAX_LEVELS];    /* tiles of 32 pixels of the destination l */
  int32_t sums_grid_x[MEMHIP_FPN_MAX_LEVELS];      /* G_l = min(ceil(R_l / 32), MEMHIP_BN_GROUPS) */
  int32_t apply_grid_x[MEMHIP_FPN_MAX_LEVELS];     /* tiles of 64 pixels of level l */
  int32_t sums_lds_bytes;                     /* the fold's scratch: 2 x 32 x 64 floats */
  int32_t slot_floats;                        /* workspace floats per workgroup of the sums: 2 C */
  int32_t fold_grid;                          /* workgroups of the second launch of the sums */
  uint64_t ws_bytes;                          /* MEMHIP_BN_GROUPS slots */
};
typedef struct memhip_fpn_plan memhip_fpn_plan_t;
int memhip_fpn_plan(const memhip_fpn_args_t* args, memhip_fpn_plan_t* out);

/* ------------------------------------------------------------------------
 * Segmentation data chain (DSEC), image and label, batched with per-sample sizes (host draws, device arithmetic)
 * replaces Resize(ratio_range) on the image and on the label   mem/semantic_segmentation/configs/_base_/datasets/dsec.py:14
 *          RemoveHotPixelsEvs                                   mem/semantic_segmentation/backbone/EventDataset.py:566-596
 *          NormalizeEvs, ToUnit8Evs                             EventDataset.py:1339-1354, 1526-1535
 *          RandomCrop, RandomFlip, Normalize(to_rgb), Pad       dsec.py:21-24 (train), 41-44 (test)
 *          the backbone's resize_in                             mem/semantic_segmentation/backbone/mem.py:294,420
 * ------------------------------------------------------------------------
 * The resized image of sample b has its own size dims[b] = (h_b, w_b), 1 <= h_b <= max_h, 1 <= w_b <= max_w, and is stored
 * densely as [3, h_b, w_b] at element offs[b] of the working buffer: a byte offset into img_u8, a float offset into img_f32,
 * offs[b] + 3 h_b w_b <= img_elems.  A sample whose dims or offs break these rules is skipped by every kernel (nothing of it is
 * read or written).  Three entries on the caller's stream, one host struct; NULL / 0 = off; a field another entry owns is
 * ignored.  No float atomics, no host synchronisation, no allocation; B == 0 is MEMHIP_OK, nothing is read.
 *
 *   memhip_segdata_resize_hist: planes u8 [B, 3, H, W] (the rasterizer's [pos, 0, neg]) -> img_u8 at offs / dims, bilinear with
 *     half-pixel centres and clamped edges in exact integer arithmetic: output x reads the source position
 *     ((2 x + 1) W - w_b) / (2 w_b) clamped to [0, W - 1]; the two taps carry the integer weights nx, 2 w_b - nx (rows: ny of
 *     2 h_b) and the value is (sum v nx ny + 2 w_b h_b) / (4 w_b h_b), round half up, in 64-bit integers.
 *     Equal sizes give an exact copy.  hist u32 [B, 2, 256] is cleared by the call and then holds H_val, the counts of the values
 *     of channels 0 and 2 of the RESIZED image, and H_pmax, the counts of max(ch0, ch2) per pixel (integer atomics: sums do not
 *     depend on their order).  OpenCV's 8-bit INTER_LINEAR, which mmcv's imresize calls, uses 11-bit fixed-point coefficients
 *     and may differ from this exact rational form by one count in isolated pixels: unmeasured, OpenCV is not available here.
 *   memhip_segdata_norm: the three whole-image reductions of RemoveHotPixelsEvs and NormalizeEvs come from the 256 bins, which
 *     every workgroup re-reads: n, sum v, sum v^2 exactly from H_val (int64), thr = mean + num_stds * unbiased std in double;
 *     a pixel is hot iff max(ch0, ch2) > thr (strict; the reference's unravel_index on the (3, H, W) shape lands on the same
 *     (y, x) for both polarities), hot pixels are zeroed in channels 0 and 2; m = the largest non-empty bin of H_pmax not above
 *     thr, 1 when that is 0; every channel becomes (v / m) * 255.f: a correctly rounded fp32 division, then a multiply.
 *     out_f32 == 0: truncated to u8 in place in img_u8 (NormalizeEvs, ToUnit8Evs: the train chain); out_f32 == 1: stored
 *     unrounded to img_f32 at the same offs (the test chain).  Channel 1 is the rasterizer's zero plane: it is scaled like the
 *     others and is not part of the maximum.
 *   memhip_segdata_geom: crop i32 [B, 3] = {top, left, flip} (clamped into the image).  Image: in_f32 ? img_f32 : img_u8 at
 *     offs / dims -> out f32 [B, 3, net_h, net_w] in one gather: crop to (crop_h, crop_w), horizontal flip of the cropped
 *     window, swap of channels 0 and 2 (Normalize(mean 0, std 1, to_rgb=True) is only that), zero pad right / bottom to the
 *     crop size, then bilinear resize to the net size with align_corners=False and no antialias (F.interpolate's function:
 *     src = (in / out) (dst + 0.5) - 0.5 clamped at 0, taken exactly as ((2 dst + 1) in - out) / (2 out): the tap is the integer
 *     quotient, the weight the remainder rounded once to fp32, then w0y (w0x a + w1x b) + w1y (w0x c + w1x d) in fp32; aten's
 *     fp32 evaluation of src is off by up to in * 2^-23, and the weight with it).  torchvision >= 0.17 would antialias this downscale; the tensor
 *     behaviour current when the reference was written is taken.  Labels: labels u8 [B, H, W] -> label_out u8 [B, crop_h,
 *     crop_w]: nearest resize to dims[b] (source index min(dst * src / dst_size, src - 1), integer; OpenCV's INTER_NEAREST
 *     computes the index in double: unmeasured as above), the same crop and flip, pad 255.  out NULL or label_out NULL: that
 *     half is off. */
struct memhip_segdata_args {
  int32_t B, H, W;                   /* the source canvas of planes and labels */
  int32_t max_h, max_w;              /* upper bounds of dims */
  int32_t crop_h, crop_w;            /* _geom */
  int32_t net_h, net_w;              /* _geom */
  int32_t out_f32;                   /* _norm: 0 = u8 in place, 1 = f32 to img_f32 */
  int32_t in_f32;                    /* _geom: the image is read from img_f32 */
  int32_t reserved0;
  double num_stds;                   /* _norm */
  const uint8_t* planes;             /* device u8 [B, 3, H, W]: _resize_hist */
  const int64_t* offs;               /* device i64 [B] */
  const int32_t* dims;               /* device i32 [B, 2] */
  uint8_t* img_u8;                   /* device: the working image, u8 */
  float* img_f32;                    /* device: the working image, f32 */
  int64_t img_elems;                 /* elements of the working buffer in use */
  uint32_t* hist;                    /* device u32 [B, 2, 256] */
  const int32_t* crop;               /* device i32 [B, 3]: _geom */
  float* out;                        /* device f32 [B, 3, net_h, net_w]: _geom */
  const uint8_t* labels;             /* device u8 [B, H, W]: _geom */
  uint8_t* label_out;                /* device u8 [B, crop_h, crop_w]: _geom */
};
typedef struct memhip_segdata_args memhip_segdata_args_t;
int memhip_segdata_resize_hist(const memhip_segdata_args_t* args, memhip_stream_t stream);
int memhip_segdata_norm(const memhip_segdata_args_t* args, memhip_stream_t stream);
int memhip_segdata_geom(const memhip_segdata_args_t* args, memhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MEMHIP_H */
