/*
 * empanada_hip.h -- C ABI of libempanada_hip.so, the MI355X (gfx950) engine
 * behind the empanada panoptic-inference hot path.
 *
 * The reference (volume-em/empanada-napari) has no FFI: its boundary for this
 * path is the Python API of empanada/inference/engines.py and
 * empanada_napari/inference.py.  Each entry point below replaces the work one
 * of those Python functions hands to torch / torch.jit / numba, and cites it.
 * The Python mirror of the reference classes (empanada-napari_amd/engines.py,
 * inference.py) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller;
 *     h_* is a HOST pointer; `stream` is a hipStream_t passed as void*.
 *   - return value: 0 on success, a negative emp_status otherwise; no C++
 *     exception crosses the ABI; emp_last_error() returns a static message.
 *   - nothing here synchronises the device except where stated (functions that
 *     return a host count).
 *   - dense float outputs use the reference's NCHW fp32 layout; label maps are
 *     int32 or int64 as stated per function.
 */
#ifndef EMPANADA_HIP_H
#define EMPANADA_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define EMP_API __attribute__((visibility("default")))
#else
#define EMP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  EMP_OK = 0,
  EMP_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  EMP_ERR_HIP = -2,       /* a HIP runtime call failed */
  EMP_ERR_STATE = -3,     /* call order (missing parameter, not finalized) */
  EMP_ERR_NOMEM = -4
} emp_status;

EMP_API const char* emp_last_error(void);
EMP_API int emp_abi_version(void);
/* number of visible HIP devices, or a negative emp_status */
EMP_API int emp_device_count(void);

/* ------------------------------------------------------------------------
 * 1. Network forward (hot loop 1)
 *    replaces: model(image, render_steps, interpolate_ins) as called from
 *    PanopticDeepLabRenderEngine.infer, empanada/inference/engines.py:248-255,
 *    i.e. QuantizablePanopticDeepLabPR.forward,
 *    empanada/models/quantization/panoptic_deeplab.py:238-250, or (arch 1)
 *    QuantizablePanopticBiFPNPR.forward, quantization/panoptic_bifpn.py:147-161
 *    (H and W must then be multiples of 128).
 * ---------------------------------------------------------------------- */
typedef struct emp_pdl emp_pdl_t;

typedef struct {
  int32_t num_classes;            /* semantic channels C (1 = binary/sigmoid)          */
  int32_t stage4_stride;          /* 16 (layer4 dilated) or 32                         */
  int32_t decoder_channels;       /* 256                                               */
  int32_t aspp_channels;          /* 0 -> decoder_channels                             */
  int32_t n_stages;               /* number of low-level decoder stages (<=3)          */
  int32_t low_level_stages[3];    /* pyramid index per stage (1..3)                    */
  int32_t low_level_proj_sem[3];  /* projected channels, semantic decoder              */
  int32_t low_level_proj_ins[3];  /* projected channels, instance decoder              */
  int32_t atrous_rates[3];
  int32_t ins_decoder;            /* 1: separate instance decoder                      */
  int32_t num_fc;                 /* PointRend MLP depth (3)                           */
  int32_t subdivision_num_points; /* 8192                                              */
  int32_t arch;                   /* 0 PanopticDeepLabPR (MitoNet_v1), 1 PanopticBiFPNPR (MitoNet_v1_mini)  */
  int32_t fpn_dim;                /* BiFPN width (128)                                 */
  int32_t fpn_layers;             /* BiFPN depth (3)                                   */
  /* Round 4 -- the encoder.  0: ResNet50 (encoders/resnet.py:143-215).  1: a four-stage RegNet
   * (encoders/regnet.py:38-160; quantization/encoders/__init__.py exports regnetx_6p4gf and regnety_6p4gf): 3x3
   * stride-2 stem of rn_stem channels, stage i = rn_depths[i] bottleneck blocks of width rn_widths[i] with
   * rn_groups[i] groups in the 3x3, the first block of a stage at stride rn_strides[i], rn_se != 0 with the reference's
   * per-pixel squeeze-excite gate (blocks.py:35-50).  A RegNet network starts, like every network since round 6, in the
   * fp16x3 mode (emp_pdl_precision reports 2: heads within 1e-3 of the reference's fp32 forward in the max norm;
   * emp_pdl_set_precision(net, 1) is the exact fp32 mode: 1e-4); emp_pdl_set_precision(net, 0) or EMP_PRECISION=fp16
   * put it on the fp16 engine -- generic implicit-GEMM convolutions, the grouped 3x3 one launch per group, 4-5x the
   * rate, heads within ~0.6e-3 .. 1.4e-3 (rms) of the fp32 forward. */
  int32_t encoder;
  int32_t rn_stem;
  int32_t rn_widths[4];
  int32_t rn_depths[4];
  int32_t rn_groups[4];
  int32_t rn_strides[4];
  int32_t rn_se;
} emp_pdl_config;

EMP_API int emp_pdl_create(const emp_pdl_config* cfg, emp_pdl_t** out);
EMP_API void emp_pdl_destroy(emp_pdl_t* net);

/* Folded fp32 parameter of one convolution, by the reference's module path
 * (e.g. "encoder.layer1.0.conv1"); h_w is OIHW (or (O,I,1) for the PointRend
 * Conv1d layers), h_b has shape[0] entries or is NULL (zero bias).  BatchNorm
 * is already folded by the host (weights.fold_state_dict). */
EMP_API int emp_pdl_set_param(emp_pdl_t* net, const char* name, const float* h_w,
                      const int64_t* shape, int ndim, const float* h_b);
/* Packs fp16 weights on the device; fails if a parameter is missing. */
EMP_API int emp_pdl_finalize(emp_pdl_t* net);
/* Precision of the forward, chosen BEFORE emp_pdl_finalize.  ROUND 6: the default is 2, the fp16x3 MODE -- the one that
 * meets the contract (float heads within 1e-3 of the reference's fp32 forward, max norm); 0, the fp16 ENGINE, is the explicit
 * throughput opt-in (emp_pdl_set_precision(net, 0) or EMP_PRECISION=fp16: 3x the rate, ~1e-3 rms / ~5e-3 max), and it is
 * what bench.py's headline `value` measures because BASELINE's metric is quoted in fp16.
 * Round 4 -- 0 the fp16 engine; 1 the fp32 REFERENCE
 * MODE (csrc/ref32.hip): every map and weight fp32, products on the exact fp32 matrix pipe (v_mfma_f32_32x32x2_f32), no
 * layer fusion.  The reference runs this path in fp32 (empanada/inference/engines.py:248-255: the model in eval, no
 * autocast); in this mode the float heads meet the north star's 1e-3 in the MAX norm (~1e-5 measured), at roughly a
 * tenth of the fp16 engine's rate -- it is the device-side comparator, not the bench.  Same entry points and output
 * tensors; emp_pdl_tap is not available (emp_pdl_tap_raw hands out every fp32 NHWC map of the last forward by name).
 * The environment variable EMP_PRECISION=fp32 selects it for networks that do not call this.
 * Round 5 (ABI version 3) -- 2: the fp16x3 MODE: the fp32 mode's graph, maps and weights, every convolution on the FP16
 * matrix pipe with both operands split into fp16 pairs and three MFMAs per product into an fp32 accumulator
 * (csrc/conv16x3.hip; weights split once at emp_pdl_finalize).  Heads within 1e-3 of the reference's fp32 forward in the
 * MAX norm on every tile and weight draw tested (2.4e-5 worst on the centre map), at ~2.5x the fp32 mode's rate: the mode
 * for results that must meet the tolerance as written, and since round 6 the default.  EMP_PRECISION=fp16 / fp32 / fp16x3
 * selects a mode for networks that do not call this. */
EMP_API int emp_pdl_set_precision(emp_pdl_t* net, int precision);
EMP_API int emp_pdl_precision(const emp_pdl_t* net);
/* Number of parameters the network expects, and the name of the i-th one. */
EMP_API int emp_pdl_num_params(const emp_pdl_t* net);
EMP_API const char* emp_pdl_param_name(const emp_pdl_t* net, int i);

/* (Re)allocates the activation arena for batches up to N x H x W.  Called
 * implicitly by emp_pdl_forward when the shape grows; call it explicitly
 * before capturing the forward into a hipGraph. */
EMP_API int emp_pdl_reserve(emp_pdl_t* net, int N, int H, int W);
EMP_API size_t emp_pdl_arena_bytes(const emp_pdl_t* net);

typedef enum { EMP_IMG_F32 = 0, EMP_IMG_U8 = 1, EMP_IMG_U16 = 2 } emp_image_dtype;

/* d_image: (N,H,W) single channel, H % 16 == 0 and W % 16 == 0
 *   EMP_IMG_F32: already normalised (Preprocessor + factor_pad output);
 *   EMP_IMG_U8/U16: raw tile, normalised in the stem as (x - sub) * mul
 *   (empanada_napari/utils.py:153-165).
 * Outputs (fp32, NCHW):
 *   d_sem_logits (N, C, H*2^(rs-2), W*2^(rs-2))
 *   d_ctr_hmp    (N, 1, h, w), d_offsets (N, 2, h, w) with h,w = H/4,W/4, or
 *   H,W when interpolate_ins != 0 (bilinear x4, align_corners=True).  */
EMP_API int emp_pdl_forward(emp_pdl_t* net, const void* d_image, int image_dtype,
                    float sub, float mul, int N, int H, int W,
                    int render_steps, int interpolate_ins,
                    float* d_sem_logits, float* d_ctr_hmp, float* d_offsets,
                    void* stream);

/* Same forward with `factor_pad` (postprocess.py:25-36) fused into the stem: d_image is the tight (N,vh,vw) image,
 * the network runs at the padded size H x W (multiples of 16, H >= vh, W >= vw) and pixels outside vh x vw are zero
 * AFTER normalisation, as in the reference.  Outputs have the padded size. */
EMP_API int emp_pdl_forward_padded(emp_pdl_t* net, const void* d_image, int image_dtype,
                    float sub, float mul, int N, int vh, int vw, int H, int W,
                    int render_steps, int interpolate_ins,
                    float* d_sem_logits, float* d_ctr_hmp, float* d_offsets,
                    void* stream);

/* Algorithmic FLOPs (2*MAC) of one forward at this shape: conv/GEMM work only. */
EMP_API double emp_pdl_flops(const emp_pdl_t* net, int N, int H, int W, int render_steps);

/* Live timing of the dominant kernel class (the 256x256 implicit-GEMM conv tile): while enabled every such
 * launch is bracketed by HIP events on the forward's stream; emp_pdl_profile_read waits for them, returns the summed
 * duration, the algorithmic FLOPs (2*MAC) and the number of launches since the last read, and resets.  Used by
 * bench.py for the roofline block; no reference counterpart. */
EMP_API int emp_pdl_profile(emp_pdl_t* net, int enable);
EMP_API int emp_pdl_profile_read(emp_pdl_t* net, double* ms_total, double* flops_total, int* launches);

/* Parity/debug taps: keep every intermediate activation addressable by name
 * after a forward ("stem", "encoder.layer1.0", ..., "semantic_x").  Returns
 * the device pointer (fp16 NHWC) and shape {N,H,W,C,ld}. */
EMP_API int emp_pdl_tap(emp_pdl_t* net, const char* name, void** d_ptr, int64_t shape5[5]);
EMP_API int emp_pdl_num_taps(const emp_pdl_t* net);
/* the fp32 buffers of the last forward that are not NHWC fp16 maps ("semantic_head.out": the coarse logits the
 * PointRend subdivision starts from, (N,C,H/4,W/4); "ins_center.out", "ins_xy.out" when interpolate_ins): device
 * pointer + size in bytes */
EMP_API int emp_pdl_tap_raw(emp_pdl_t* net, const char* name, void** d_ptr, int64_t* bytes);
/* Parity/debug only, fp32 and fp16x3 modes: the buffers the LAST forward made, in the order it made them (the intermediate
 * maps of QuantizablePanopticDeepLabPR.forward / QuantizablePanopticBiFPNPR.forward, quantization/panoptic_deeplab.py:194-250,
 * panoptic_bifpn.py:147-161, which the reference never names; no reference counterpart).  emp_pdl_tap_raw serves a buffer by
 * name whichever forward left it; this list holds what the last one wrote, with its geometry.  Entry i -> name, kind, device
 * pointer, shape5 = {N, H, W, C, ld} and fmt (0 fp32, 1 hl32: csrc/conv16x3p.hip's hi / lo rows, ld in channels).  kind:
 *   "map"                          NHWC rows of ld floats, C of them written; channels [C, ld) are padding that must read zero
 *   "pooled" "poolfeat" "bias_n"   N rows of C floats
 *   "out"                          a head's planes, NCHW (N, C, H, W) -- the pointer the forward WROTE: the caller's tensor for
 *                                  ins_center / ins_xy without interpolate_ins
 *   "part"                         the fused head's partial sums (ld cout tiles, N, H * W, C)
 *   "pr.keys" (N, W) uint32, "pr.topk" W floats of scratch, "pr.idx" (N, W) int32, "pr.x" W rows of C floats: what the buffers
 *             can hold -- a step whose plane or k is smaller packs its keys as (N, plane), its indices as (N, k), its rows N * k
 *   "pr.sem"  NCHW (N, C, H, W) logits of an inner subdivision step
 * The strings live until the next forward or emp_pdl_destroy.  emp_pdl_num_taps / emp_pdl_tap are unchanged. */
EMP_API int emp_pdl_num_maps32(const emp_pdl_t* net);
EMP_API int emp_pdl_map32(const emp_pdl_t* net, int i, const char** name, const char** kind, void** d_ptr, int64_t shape5[5], int* fmt);
/* device-to-device copy on `stream` (lets a host language without a HIP binding read a tap) */
EMP_API int emp_copy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
EMP_API const char* emp_pdl_tap_name(const emp_pdl_t* net, int i);

/* ------------------------------------------------------------------------
 * 2. Building-block operators (used by the network, exported for parity
 *    tests and for callers that run their own graph)
 * ---------------------------------------------------------------------- */

/* NHWC fp16 implicit-GEMM convolution on MFMA, fp32 accumulate, fused
 * bias + per-image bias + residual + ReLU.  replaces: nn.Conv2d(+folded
 * BatchNorm)(+ReLU)(+skip add), e.g. encoders/resnet.py:109-129.
 *   d_in  : (N,H,W,in_ld) fp16, the conv reads channels [0,Cin); Cin % 64 == 0
 *   d_w   : (Cout, KH*KW, Cin) fp16
 *   d_bias: (Cout) fp32 or NULL;  d_bias_n: (N,Cout) fp32 or NULL
 *   d_res : (N,Ho,Wo,res_ld) fp16 or NULL
 *   d_out : (N,Ho,Wo,out_ld) fp16; writes channels [0,Cout); Cout % 8 == 0
 *   variant: 0 = automatic.  Otherwise staging (bits 0-3: 1 registers | 2 LDS-DMA | 3 LDS-DMA + LDS-transposed epilogue)
 *     + 16 * tile (1 128x128 | 2 128x64 | 3 64x64 | 4 256x256 | 5 half tile 128x256 / 256x128 | 6 64->64 3x3 with
 *     register weights | 7 64x64 with a deep LDS-DMA ring, the batch-1 path) + 256 * K-walk group; every tile gives
 *     bit-identical results (same K order) at the default K-walk group, the parity tests force each one.  A K-walk group of
 *     its own is another summation order: the same bounds, not the same bits (tests/test_gpu_f16_range.py: 512 -> 128 3x3,
 *     groups of 2 slabs against the default 4).
 *     + (1 << 20): d_w is the 256x256 tile's PACKED weight image (emp_conv256_pack_weights, round 5) -- that tile, its
 *     default K walk, the same bits out. */
EMP_API int emp_conv2d_nhwc_f16(const void* d_in, int N, int H, int W, int Cin, int in_ld,
                        const void* d_w, const float* d_bias, const float* d_bias_n,
                        const void* d_res, int res_ld,
                        void* d_out, int out_ld, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int relu,
                        int variant, void* stream);

/* Every ConvParams feature that the network reaches and emp_conv2d_nhwc_f16 / emp_conv1x1_dual_nhwc_f16 cannot express, for
 * op-level tests and tuning (replaces the same nn.Conv2d + folded BN + activation, encoders/resnet.py:109-129; the store variants
 * replace the transposed convolutions of blocks.py:154-171 and the launches the scheduler merges).  Everything
 * emp_conv2d_nhwc_f16 takes (act: 0 none, 1 ReLU, 2 SiLU; `variant` unchanged: staging + 16 * tile, K-walk group << 8,
 * 256-tile DMA mode << 16, packed image << 20), plus
 *   d_in2 .. : optional second source K-concatenated behind the first, as emp_conv1x1_dual_nhwc_f16 (d_w rows [KH*KW*Cin | Cin2])
 *   ps_cout  : > 0: Cout == 4 * ps_cout, cout block q = dy * 2 + dx of pixel (y, x) is stored at pixel (2y + dy, 2x + dx) of a
 *              (N, 2Ho, 2Wo, out_ld) map -- a k2 s2 transposed convolution as four 1x1 convolutions
 *   d_out2 ..: optional second destination: couts [split, Cout) go to d_out2 (channel 0 = cout `split`); with d_out3 couts
 *              [split, split3) go to d_out2 and [split3, Cout) to d_out3; split, split3 % 8 == 0 (% 256 on the 256x256 tile)
 *   d_next_w : optional back-to-back 1x1 fused into the 256x256 tile (Cout == 256, >= 192 pixel tiles): (next_cout, Cout) fp16,
 *              d_next_out (N,Ho,Wo,next_ld) = relu(d_next_w . out + d_next_b), computed from the stored fp16 tile; next_cout == 64
 * A combination the launchers refuse returns their error (emp_last_error).  Not a hot-path call. */
EMP_API int emp_conv2d_nhwc_f16_ex(const void* d_in, int N, int H, int W, int Cin, int in_ld,
                        const void* d_w, const float* d_bias, const float* d_bias_n,
                        const void* d_res, int res_ld,
                        void* d_out, int out_ld, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act, int variant,
                        const void* d_in2, int H2, int W2, int Cin2, int in2_ld, int stride2,
                        int ps_cout,
                        void* d_out2, int out2_ld, int split, void* d_out3, int out3_ld, int split3,
                        const void* d_next_w, const float* d_next_b, void* d_next_out, int next_cout, int next_ld,
                        void* stream);

/* The same convolution with `groups` groups on the fp16 engine (nn.Conv2d(groups=g), the 3x3 of a RegNet bottleneck:
 * encoders/regnet.py:51-77), for op-level tests and tuning: Cin / Cout describe ONE group -- Cin the group's input channels padded
 * to a multiple of 64, the padding meeting zero weights -- group g reads channels [g * gs_in, g * gs_in + Cin) of d_in, the
 * weights d_w + g * gs_w halfs ((Cout, KH*KW, Cin) each), and writes channels [g * gs_out, g * gs_out + Cout) of d_out (bias
 * likewise); no residual, per-image bias or second source.  tile: 0 the launcher's choice, 1 the 128x128 instantiation,
 * 2 the 128x64 one (same K order: the same bits).  Not a hot-path call. */
EMP_API int emp_conv2d_grouped_nhwc_f16(const void* d_in, int N, int H, int W, int Cin, int in_ld,
                        const void* d_w, const float* d_bias, void* d_out, int out_ld, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act,
                        int groups, int gs_in, long long gs_w, int gs_out, int tile, void* stream);

/* Packed weight image for the 256x256 convolution tile (round 5; csrc/conv_igemm256.hip pack256_kernel): the network
 * (emp_pdl_*) makes one per layer at the first launch that takes the tile.  Every 1 KiB piece an LDS-DMA instruction moves
 * (16 cout rows x 32 channels of one K step) is contiguous in the image, in the kernel's K-walk order, so the instruction
 * fetches whole 128-byte lines.  replaces: nothing in the reference (nn.Conv2d weights, resnet.py:109-129, re-laid out).
 *   d_w      : (Cout, KT * Cin + Cin2) fp16 -- the weights of emp_conv2d_nhwc_f16 (KT = KH*KW; Cin2 = the K-concatenated
 *              second source's channels, 0 if none); Cout % 256 == 0, Cin % 32 == 0, Cin2 % 32 == 0
 *   d_packed : the same number of halfs */
EMP_API int emp_conv256_pack_weights(const void* d_w, void* d_packed, int Cout, int KT, int Cin, int Cin2, void* stream);

/* The convolution of the fp32 REFERENCE MODE (round 4, csrc/ref32.hip; emp_pdl_set_precision): NHWC fp32 maps, fp32
 * weights (Cout, KH*KW, Cin) with Cin % 16 == 0 (pad with zero weights), every product on the exact fp32 matrix pipe
 * (v_mfma_f32_32x32x2_f32).  replaces nn.Conv2d(+folded BatchNorm)(+ReLU / SiLU)(+skip add) exactly as the reference
 * computes it (fp32, engines.py:248-255).  act: 0 none, 1 ReLU, 2 SiLU; other arguments as emp_conv2d_nhwc_f16. */
EMP_API int emp_conv2d_nhwc_f32(const float* d_in, int N, int H, int W, int Cin, int in_ld,
                        const float* d_w, const float* d_bias, const float* d_bias_n,
                        const float* d_res, int res_ld,
                        float* d_out, int out_ld, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act, void* stream);

/* The same convolution in the `fp16x3` precision mode (round 5, csrc/conv16x3.hip; emp_pdl_set_precision(net, 2)): the
 * same fp32 operands, every operand split into an fp16 pair x = hi + lo on its way into LDS and every product computed as
 * w_lo.x_hi + w_hi.x_lo + w_hi.x_hi on the FP16 matrix pipe into an fp32 accumulator -- the reference's fp32 result
 * (engines.py:248-255) at three fp16 MFMAs per product instead of sixteen fp16-MFMA times on the fp32 pipe.  Operand range: a
 * pair holds its operand to 2^-22 relative for 2^-3 <= |x| < 65520, to an absolute 2^-25 below 2^-3 (lo is an fp16 subnormal;
 * the matrix pipe keeps subnormals), is zero from 2^-25 down and not finite at and above 65520; a term w x is therefore off by
 * at most max(2^-22 |x|, 2^-25) |w| + |x| max(2^-22 |w|, 2^-25) + 2^-22 |w x| (tests/test_gpu_x3_range.py holds every output
 * element of every entry below to the sum of these).  groups > 1: Cout and Cin are per group (Cin = cin_g padded to 16), as emp_conv2d_grouped_nhwc_f32;
 * groups == 1: cin_g = 0.  Values at or above 65520 in magnitude give NaN (0 behind a ReLU). */
EMP_API int emp_conv2d_nhwc_f16x3(const float* d_in, int N, int H, int W, int Cin, int in_ld,
                        const float* d_w, const float* d_bias, const float* d_bias_n,
                        const float* d_res, int res_ld,
                        float* d_out, int out_ld, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act,
                        int groups, int cin_g, void* stream);

/* Round 6 (ABI version 5) -- every variant of the fp16x3 convolution that the network reaches and the entry above cannot
 * express, for op-level tests and tuning (replaces the same nn.Conv2d, resnet.py:109-129 / aspp.py:51-103 / heads.py:12-15):
 *   wmode    : 0 fp32 weights split in the kernel; 1 weights pre-split into fp16 pairs (what emp_pdl_finalize makes);
 *              2 pairs + the split-role kernel's LDS-DMA weight image (long K, Cin % 32 == 0);
 *              + 4: split-K allowed -- a long-K launch of fewer than 128 workgroups (few pixels: ONE 1024^2 tile's ASPP branch) runs
 *              S <= 8 workgroups per tile over K / S each, fp32 partial sums added in ascending order by a finish pass (what the
 *              network does at small batches; the result differs from the unsplit one by fp32 summation order only)
 *   d_in2 .. : optional second source K-concatenated behind the first -- a 1x1 convolution of d_in2 (N, H2, W2, in2_ld) at
 *              stride2 summed into the same accumulators (a bottleneck's projection shortcut folded into conv3); d_w rows are
 *              then [KH*KW*Cin | Cin2] long
 *   d_head_w : optional fused 1x1 head (heads.py:14): (head_c, Cout) fp32; the activation map is not stored, d_head_out
 *              receives (N, head_c, Ho*Wo) = head_w . relu(conv) + d_head_b; head_c <= 4, act must be 1
 *   out_fmt  : 0 fp32 rows; 1 `hl32` rows (below).
 * Allocates and frees its temporaries and synchronises the stream: not a hot-path call. */
EMP_API int emp_conv2d_nhwc_f16x3_ex(const float* d_in, int N, int H, int W, int Cin, int in_ld,
                        const float* d_w, const float* d_bias, const float* d_bias_n,
                        const float* d_res, int res_ld,
                        void* d_out, int out_ld, int out_fmt, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act, int wmode,
                        const float* d_in2, int H2, int W2, int Cin2, int in2_ld, int stride2,
                        const float* d_head_w, const float* d_head_b, int head_c, float* d_head_out,
                        void* stream);

/* Round 6 -- the `hl32` map format and the 256 x 256 fp16x3 convolution over it (csrc/conv16x3p.hip).  An hl32 map keeps a
 * value x of the fp32 graph as the fp16 pair the fp16x3 product needs -- hi = fp16(x), lo = fp16(x - hi); hi + lo is x to
 * 2^-22 |x| for 2^-3 <= |x| < 65520, to 2^-25 absolute below 2^-3 (subnormal lo halves are kept, -0.0 keeps its sign), exactly 0
 * for |x| <= 2^-25, not finite from 65520 -- split ONCE by the producer: a row of C channels (C % 32 == 0) is C / 32 blocks of 128 bytes, each 32 hi halfs
 * followed by 32 lo halfs; rows are 2 * ld halfs apart (the fp32 map's 4 bytes per element).  The networks of precision 2 keep
 * the stride-16 region (ResNet layer3 / layer4, ASPP: resnet.py:109-129, aspp.py:51-103) in this format, so that the 128 bytes a
 * pixel contributes to a K step of 32 channels are one cache line and one LDS row, fetched by LDS-DMA.
 *   emp_hl32_from_f32 / emp_hl32_to_f32 : (rows, C) fp32 rows of in_ld floats <-> hl32 rows (ld in channels)
 *   emp_x3p_pack_weights : (Cout, K) fp32, K = KH*KW*Cin walked tap-major, Cout % 256 == 0, K % 32 == 0 -> the kernel's packed
 *                          image of 2 * Cout * K halfs ([cout tile][K step][lo pieces | hi pieces], rows permuted and chunks
 *                          swizzled as they lie in LDS)
 *   emp_conv2d_hl32_f16x3 : the convolution; d_in hl32, d_wimg the packed image, res_fmt / out_fmt 0 fp32 rows or 1 hl32
 *                          rows; Cout % 256 == 0, Cin % 32 == 0, KH*KW*Cin >= 128; the same three fp16 MFMAs per product in the
 *                          same K order as emp_conv2d_nhwc_f16x3: bit-identical results on the same operands. */
EMP_API int emp_hl32_from_f32(const float* d_in, void* d_out, int64_t rows, int C, int in_ld, int out_ld, void* stream);
EMP_API int emp_hl32_to_f32(const void* d_in, float* d_out, int64_t rows, int C, int in_ld, int out_ld, void* stream);
EMP_API int emp_x3p_pack_weights(const float* d_w, void* d_img, int Cout, int K, void* stream);
EMP_API int emp_conv2d_hl32_f16x3(const void* d_in, int N, int H, int W, int Cin, int in_ld,
                        const void* d_wimg, const float* d_bias, const float* d_bias_n,
                        const void* d_res, int res_ld, int res_fmt,
                        void* d_out, int out_ld, int out_fmt, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act, void* stream);
/* The same convolution with split-K allowed (what the network does below the plane region's batch threshold: the merged 3x3 ASPP
 * branches of ONE 1024^2 tile are 32 workgroups over 576 K steps): with d_scratch of scratch_bytes (S * M * Cout * 4 needed; 64 MiB
 * covers every launch the rule splits) a launch of fewer than 128 workgroups runs S <= 8 workgroups per tile over K / S each (raw fp32
 * partial sums), and a finish pass adds them in ascending order, then bias / bias_n / residual / activation -- the unsplit result up to
 * fp32 summation order.  d_out2 (optional): couts [split2, Cout) go there (split2 % 256 == 0), as the network's merged launches.
 * Launches the rule does not split run exactly as emp_conv2d_hl32_f16x3.  No allocation, no synchronisation. */
EMP_API int emp_conv2d_hl32_f16x3_ksplit(const void* d_in, int N, int H, int W, int Cin, int in_ld,
                        const void* d_wimg, const float* d_bias, const float* d_bias_n,
                        const void* d_res, int res_ld, int res_fmt,
                        void* d_out, int out_ld, int out_fmt, void* d_out2, int out2_ld, int split2, int Cout,
                        int KH, int KW, int stride, int pad, int dil, int act,
                        void* d_scratch, int64_t scratch_bytes, void* stream);

/* Round 6 -- the depthwise-separable block of the fp16x3 mode as ONE launch (csrc/sepconv_x3.hip): replaces
 * nn.Conv2d(C,C,k,groups=C,padding=k/2,bias=False) -> nn.Conv2d(C,Cout,1) -> folded BatchNorm -> ReLU / SiLU (models/blocks.py:15-33;
 * decoders/panoptic_deeplab.py:68-80, heads.py:12-15) and, with d_head_w, the head's final 1x1 (heads.py:14) on fp32 NHWC maps.
 * The depthwise half runs in fp32 (taps ky-major / kx-minor, an fmaf chain from 0); its result goes to LDS as the fp16 pair
 * hi + lo and meets the pointwise weights (hi + lo) in three fp16 MFMAs per product, fp32 accumulate from the bias.
 *   emp_sepconv_x3_pack : d_dw (k*k, C) fp32 taps, d_pw (Cout, C) fp32 -> d_dw_packed (k*k*C floats), d_pw_packed (2*C*Cout halfs)
 *   emp_sepconv_x3_nhwc_f32 : C % 32 == 0, 64 <= C <= 448, Cout 128 or 256, k 5 (or 3 without a head), act 0 / 1 / 2;
 *                          exactly one of d_out (N,H,W,out_ld) and the head output d_head_out (N, head_c, H*W), head_c <= 2 */
EMP_API int emp_sepconv_x3_pack(const float* d_dw, const float* d_pw, int ks, int C, int Cout,
                        float* d_dw_packed, void* d_pw_packed, void* stream);
EMP_API int emp_sepconv_x3_nhwc_f32(const float* d_in, int N, int H, int W, int C, int in_ld,
                        const float* d_dw_packed, const void* d_pw_packed, const float* d_bias, int Cout, int act,
                        float* d_out, int out_ld,
                        const float* d_head_w, const float* d_head_b, int head_c, float* d_head_out,
                        int ks, void* stream);

/* The same convolution with `groups` groups (nn.Conv2d(groups=g), the 3x3 of a RegNet bottleneck:
 * empanada/models/encoders/regnet.py:51-77 via blocks.py:134-153): group g reads input channels [g * cin_g, g * cin_g +
 * Cin16) -- Cin16 = cin_g padded to a multiple of 16, the padding meeting zero weights, so a row of the input must hold
 * (groups - 1) * cin_g + Cin16 floats -- and writes output channels [g * cout_g, (g + 1) * cout_g); weights
 * (groups * cout_g, KH*KW, Cin16), bias (groups * cout_g). */
EMP_API int emp_conv2d_grouped_nhwc_f32(const float* d_in, int N, int H, int W, int groups, int cin_g, int Cin16, int in_ld,
                        const float* d_w, const float* d_bias, float* d_out, int out_ld, int cout_g,
                        int KH, int KW, int stride, int pad, int dil, int act, void* stream);

/* out = act( in . W[:, :Cin] + in2(strided) . W[:, Cin:] + bias ): a 1x1 convolution whose reduction continues over a
 * second tensor sampled with stride2.  replaces the tail of a ResNet bottleneck with a projection shortcut,
 * `out = relu(bn3(conv3(x)) + downsample(identity))`, empanada/models/encoders/resnet.py:109-129 with
 * downsample = Conv2d(1x1, stride) + BN (:176-181): both branches accumulate in fp32 in one launch, the shortcut map is
 * never written.  d_w (Cout, Cin + Cin2) fp16, rows K-contiguous; in (N,H,W,in_ld), in2 (N,H2,W2,in2_ld) with
 * (H-1)*stride2 < H2; Cin, Cin2 multiples of 64. */
EMP_API int emp_conv1x1_dual_nhwc_f16(const void* d_in, int N, int H, int W, int Cin, int in_ld, const void* d_in2,
                              int H2, int W2, int Cin2, int in2_ld, int stride2, const void* d_w,
                              const float* d_bias, void* d_out, int out_ld, int Cout, int relu, int variant,
                              void* stream);

/* NHWC fp16 depthwise KxK convolution (K in {3,5}, stride 1, pad K/2, no bias), fp32 accumulate.
 * replaces nn.Conv2d(C, C, K, groups=C, bias=False): the first half of the decoder's separable convs
 * (models/blocks.py separable conv, models/decoders/bifpn.py SeparableConv2d).
 *   d_w: (K*K, C) fp16;  C % 64 == 0 */
EMP_API int emp_dwconv_nhwc_f16(const void* d_in, int N, int H, int W, int C, int in_ld,
                        const void* d_w, int K, void* d_out, int out_ld, void* stream);

/* Fused separable convolution: y = act(pointwise(depthwise5x5(x)) + bias), and optionally the
 * 1x1 head on top of it (head_c in 1..4) so that y never reaches HBM.
 * replaces the 'depthwise_separable_conv' blocks of the Panoptic-DeepLab decoder / heads
 * (models/decoders/panoptic_deeplab.py fuse convs, models/heads/panoptic_deeplab.py head.0 -> head.1).
 *   d_in    : (N,H,W,in_ld) fp16, channels [0,C), C % 64 == 0, 128 <= C <= 512
 *   d_dw_w  : (25, C) fp16;  d_bias: (Cout) fp32 or NULL;  Cout in {128,256}
 *   d_pw_w  : the (Cout, C) pointwise weights re-ordered by emp_sepconv5x5_pack_pw (MFMA fragment order, C*Cout fp16)
 *   act     : 0 none | 1 ReLU | 2 SiLU
 *   head_c == 0: d_out (N,H,W,out_ld) fp16 receives y
 *   head_c  > 0: d_head_out (N,head_c,H,W) fp32 receives d_head_w (head_c,Cout) . y + d_head_b; d_out unused */
EMP_API int emp_sepconv5x5_pack_pw(const void* d_pw_w, int pw_ld, int C, int Cout, void* d_packed, void* stream);
EMP_API int emp_sepconv5x5_nhwc_f16(const void* d_in, int N, int H, int W, int C, int in_ld,
                        const void* d_dw_w, const void* d_pw_w, const float* d_bias,
                        int Cout, int act, void* d_out, int out_ld,
                        const float* d_head_w, const float* d_head_b, int head_c, float* d_head_out,
                        void* stream);
/* The same with a 3x3 depthwise kernel (d_dw_w [9][C]) and no head mode: depthwise 3x3 -> pointwise -> BN -> SiLU, the
 * `SeparableConv2d` after every BiFPN fusion node, empanada/models/decoders/bifpn.py:24-45 as used at :63-69,128-134. */
EMP_API int emp_sepconv3x3_nhwc_f16(const void* d_in, int N, int H, int W, int C, int in_ld, const void* d_dw_w,
                            const void* d_pw_w, const float* d_bias, int Cout, int act, void* d_out, int out_ld,
                            void* stream);

/* The separable block with an exact depthwise half (round 3; csrc/sepconv_precise.hip): where the block above rounds
 * to fp16 inside -- depthwise taps, depthwise result, pointwise weights -- was a large part of the centre heat-map's
 * distance to the fp32 reference forward (models/quantization/panoptic_deeplab.py:238-250 run in fp32).  Here the taps
 * stay fp32 on the vector pipe and the depthwise result goes to the matrix pipe as an fp16 hi + lo pair (two MFMAs per
 * product, fp32 accumulation); the pointwise weights stay fp16 (their hi + lo form bought 0.5 % of the error for a third
 * more matrix work: measured, removed).  x and y are fp16.  Operand range: both halves are round-toward-zero conversions, so the
 * pair is short of the depthwise value d by less than 2^-21 2^floor(log2 |d|) for |d| >= 2^-3, by less than an absolute 2^-24
 * below (lo is an fp16 subnormal, kept; from 2^-13 down the pair is no better than one fp16), and zero below 2^-24; from 65520 on
 * hi is +-65504, not inf, and lo carries the rest up to |d| = 131008 (gfx950's v_cvt_pkrtz_f16_f32, measured: FINDINGS 102).
 *   K       : depthwise kernel size, 5 or 3 (3: no head mode)
 *   d_dw_w  : the (K*K, C) fp32 taps re-ordered by emp_sepconvp_pack_dw (chunk-major [C/64][K*K][64] fp32)
 *   d_pw_w  : the (Cout, C) fp32 pointwise weights (row stride pw_ld) rounded to fp16 and re-ordered by
 *             emp_sepconvp_pack_pw (C*Cout fp16, MFMA fragment order)
 *   C % 64 == 0, 128 <= C <= 512, Cout in {128,256}, head_c in 0..2; other arguments as emp_sepconv5x5_nhwc_f16 */
EMP_API int emp_sepconvp_pack_dw(const void* d_dw_w, int K, int C, void* d_packed, void* stream);
EMP_API int emp_sepconvp_pack_pw(const void* d_pw_w, int pw_ld, int C, int Cout, void* d_packed, void* stream);
EMP_API int emp_sepconvp_nhwc_f16(const void* d_in, int N, int H, int W, int C, int in_ld, int K,
                        const void* d_dw_w, const void* d_pw_w, const float* d_bias,
                        int Cout, int act, void* d_out, int out_ld,
                        const float* d_head_w, const float* d_head_b, int head_c, float* d_head_out,
                        void* stream);
/* Round 4 -- the same block with the POINTWISE WEIGHTS as an fp16 hi + lo pair too (a third MFMA per product, w_lo * x_hi;
 * Cout == 128 only): the 3x3 node blocks, the decoder's fusion conv and the centre head of PanopticBiFPNPR
 * (models/quantization/panoptic_bifpn.py:147-161, decoders/bifpn.py:35-134), whose pointwise weight roundings were 65 %
 * of the weight-side error of the centre heat-map (tools/error_budget.py --arch bifpn).  emp_sepconvp_ws_pack_pw writes
 * 2*C*Cout fp16 (the hi fragments, then the lo fragments); every other argument as above. */
EMP_API int emp_sepconvp_ws_pack_pw(const void* d_pw_w, int pw_ld, int C, int Cout, void* d_packed, void* stream);
EMP_API int emp_sepconvp_ws_nhwc_f16(const void* d_in, int N, int H, int W, int C, int in_ld, int K,
                        const void* d_dw_w, const void* d_pw_w, const float* d_bias,
                        int Cout, int act, void* d_out, int out_ld,
                        const float* d_head_w, const float* d_head_b, int head_c, float* d_head_out,
                        void* stream);

/* PointRend subdivision, operator by operator (csrc/pointrend.hip; the launches emp_pdl_forward makes per render step,
 * point_rend.py:241-269 eval branch).  Exported so that each kernel is tested against a plain reference on inputs the
 * network does not produce (tests/test_gpu_pointrend_kernels.py).  Thin wrappers: no new kernel, nothing synchronises.
 *
 * emp_pr_upsample2x_keys: d_in (N,C,h,w) fp32 -> d_out (N,C,2h,2w) fp32, F.interpolate(scale_factor=2, bilinear,
 *   align_corners=False), and d_keys (N,2h*2w) uint32: the fp32 bit pattern of |v| (C == 1) or top1 - top2 over the classes
 *   (C > 1) of the up-sampled logits -- the negated uncertainty of point_rend.py:11-31, never negative.  One thread writes four
 *   consecutive outputs of a row with 16-byte stores (W % 4 == 0 and both outputs on a 16-byte boundary), 8-byte stores (odd w)
 *   or guarded 4-byte stores (any 4-byte-aligned pointers).  EMP_PR_UP2X_LEGACY=1 (read per call): the one-output kernel; the
 *   same bits.
 * emp_pr_topk_smallest: per image the k cells with the smallest keys (fp32 bit patterns of non-negative values): every key
 *   below the k-th smallest value and, among the cells equal to it, those with the lowest index.  d_idx (N,k) int32: first
 *   the cells below the k-th value in ascending order, then the tied cells in ascending order.  k == plane returns every
 *   cell; k > plane, k <= 0 or work_bytes < emp_pr_topk_work_bytes is an error and launches nothing.  The workspace needs
 *   no initialisation and may be reused by the next call on the same stream.  The keys are read twice with 16-byte loads
 *   (a histogram of their 12 leading bits, then one pass that marks the cells below the threshold bin in a bit mask and
 *   collects the keys of that bin, at most 8192 per image, from which the exact threshold is resolved); an image whose
 *   threshold bin holds more keys (a constant image) is refined on the device by two more histogram passes, without a host
 *   synchronisation, and a batch may mix both kinds.  d_keys needs 4-byte alignment only.  EMP_TOPK_LEGACY=1 (read per
 *   call): the four-pass radix select that reads the keys six times; same output, element for element.
 * emp_pr_point_features_f16 / _f32: point_sample (point_rend.py:33-60: grid_sample, bilinear, align_corners=False, zero
 *   padding) of the NHWC feature map d_feat (N,fh,fw,feat_ld; C channels used) and of the NCHW coarse logits d_coarse
 *   (N,ncls,fh,fw) fp32 at the centres of the cells d_idx (N,P) of an H2 x W2 grid (point_rend.py:131-135).  Row p of d_x0 is
 *   [C features | ncls coarse | zeros up to ld]; row p of d_x1 receives the columns [C, ld) only (the MLP's second buffer).
 *   f16: C % 8 == 0, ld % 8 == 0, C + 8 <= ld <= C + 256, ncls <= 8.
 * emp_pr_point_head: sampling + num_fc x (1x1 conv + bias + ReLU, coarse logits re-attached) + predictor + scatter in one
 *   launch, bit-identical to emp_pr_point_features_f16, num_fc x emp_conv2d_nhwc_f16 and emp_head1x1_scatter_f16.
 *   h_fc_w[f] / h_fc_b[f]: HOST arrays of num_fc device pointers, (C, ld) fp16 weights whose columns [C + ncls, ld) are zero
 *   and C fp32 biases; d_pred_w (ncls, ld) fp32, d_pred_b ncls fp32; d_out (N,ncls,plane) fp32, written at d_idx only.
 *   emp_pr_point_head_supported returns 1 for the shapes it takes -- (C, ld) = (256, 320) or (128, 192), ncls 1..8,
 *   num_fc 1..4 -- and 0 otherwise; emp_pr_point_head returns EMP_ERR_INVALID for the others.
 * emp_head1x1_scatter_f16 / _f32: out[n, c, idx[n, p]] = sum_k in[n*P + p, k] * w[c, k] + b[c] for rows of fp16 (K % 8 == 0,
 *   K <= 512) or fp32; d_w (C, K) fp32.  d_scatter_idx NULL: the row's own position p (plane >= P). */
EMP_API int emp_pr_upsample2x_keys(const float* d_in, int N, int C, int h, int w, float* d_out, uint32_t* d_keys, void* stream);
EMP_API int emp_pr_topk_work_bytes(int N, int64_t plane, size_t* h_bytes);
EMP_API int emp_pr_topk_smallest(const uint32_t* d_keys, int N, int64_t plane, int k, void* d_work, size_t work_bytes,
                                 int32_t* d_idx, void* stream);
EMP_API int emp_pr_point_features_f16(const void* d_feat, int N, int fh, int fw, int C, int feat_ld, const float* d_coarse,
                                      int ncls, const int32_t* d_idx, int P, int H2, int W2, void* d_x0, void* d_x1, int ld,
                                      void* stream);
EMP_API int emp_pr_point_features_f32(const float* d_feat, int N, int fh, int fw, int C, int feat_ld, const float* d_coarse,
                                      int ncls, const int32_t* d_idx, int P, int H2, int W2, float* d_x0, float* d_x1, int ld,
                                      void* stream);
EMP_API int emp_pr_point_head_supported(int C, int ld, int ncls, int num_fc);
EMP_API int emp_pr_point_head(const void* d_feat, int N, int fh, int fw, int C, int feat_ld, const float* d_coarse, int ncls,
                              const int32_t* d_idx, int P, int H2, int W2, const void* const* h_fc_w,
                              const float* const* h_fc_b, int num_fc, int ld, const float* d_pred_w, const float* d_pred_b,
                              float* d_out, int64_t plane, void* stream);
EMP_API int emp_head1x1_scatter_f16(const void* d_in, int N, int P, int K, int in_ld, const float* d_w, const float* d_b, int C,
                                    float* d_out, int64_t plane, const int32_t* d_scatter_idx, void* stream);
EMP_API int emp_head1x1_scatter_f32(const float* d_in, int N, int P, int K, int in_ld, const float* d_w, const float* d_b, int C,
                                    float* d_out, int64_t plane, const int32_t* d_scatter_idx, void* stream);

/* The network's glue layers, operator by operator (csrc/layers.hip, csrc/stem.hip, their fp32 twins in csrc/ref32.hip and the
 * plane region's average pool in csrc/conv16x3p.hip: every launch of emp_pdl_forward that is not a convolution).  Exported so that
 * each kernel is tested against a plain float64 reference at shapes the network does not produce
 * (tests/test_gpu_layer_kernels.py; references and error bounds in tests/layers_case.py).  Thin wrappers: no new kernel, nothing
 * synchronises, nothing allocates.  A bad argument returns EMP_ERR_INVALID and launches nothing.
 *
 * prec selects the kernel: EMP_OP_F16 the fp16 engine's (fp16 NHWC maps), EMP_OP_F32 the fp32 / fp16x3 graph's (fp32 NHWC maps),
 * EMP_OP_HL32 (emp_op_avgpool only) the plane region's hl32 map.  Maps are dense NHWC unless a row stride (`*_ld`, in elements)
 * is given; fp16 kernels move 8 channels per lane (C, strides % 8 == 0), fp32 kernels 4 (% 4 == 0); pointers 16-byte aligned.
 *
 * emp_op_stem7x7: d_img (N,vh,vw) of image_dtype -> d_out (N,H/2,W/2,64): 7x7 stride-2 pad-3 conv + bias + ReLU of the image
 *   normalised as (v - sub) * mul (EMP_IMG_U8 / U16; EMP_IMG_F32 is taken as it is) and THEN zero-padded from vh x vw to H x W
 *   and by the convolution.  d_w (49,64) fp32 tap-major, d_b 64.  H, W even, 1 <= vh <= H, 1 <= vw <= W.  F16: stem7x7_kernel
 *   storing fp16; F32: the same kernel storing its fp32 sums.
 * emp_op_stem_pool: the same followed by the 3x3 stride-2 pad-1 max-pool, in one launch on the matrix pipe -> d_out
 *   (N,H/4,W/4,64); H, W % 4 == 0.  F16: stem_pool_kernel_v2 (conv tile rounded to fp16 before the pool; the next tile's patch is
 *   fetched under the current tile's work), or with EMP_STEM_POOL_LEGACY=1 stem_pool_kernel, the same bits;
 *   EMP_STEM_POOL_GRID=<n> caps the workgroups of either (a test hook: the tile loop on small images); both read per call.
 *   F32: stem_pool32_kernel.
 * emp_op_stem3x3s2: 3x3 stride-2 pad-1 conv + bias + ReLU, same normalisation and padding -> d_out (N,H/2,W/2,out_ld), C
 *   channels written; d_w (9,C) fp32.  F16: stem3x3s2_f16_kernel (C % 8); F32: stem3x3s2_32_kernel (C % 4).
 * emp_op_maxpool3x3s2: 3x3 stride-2 pad-1 max-pool, -inf padding, (N,H,W,C) -> (N,H/2,W/2,C); H, W even.  Exact.
 * emp_op_fuse_combine: out = ca * r(a) + cb * b (+ cc * c when d_c is not NULL), b, c, out (N,H,W,C).  mode 0: a is (N,H/2,W/2,C)
 *   and r the nearest x2 up-sampling (H, W even); mode 1: a is (N,2H,2W,C) and r the 3x3 stride-2 pad-1 max-pool.  F16: rows of
 *   d_out out_ld apart (0: C); d_out_lo not NULL: the fp32 sum leaves as an fp16 pair, hi = fp16(v) to d_out and lo = fp16(v - hi)
 *   to d_out_lo (same stride).  F32: fuse_combine32_kernel, dense, d_out_lo NULL and out_ld 0 or C.
 * emp_op_bilinear_ac_nhwc: F.interpolate(bilinear, align_corners=True) of C channels of (N,h,w,in_ld) into C channels of
 *   (N,H,W,out_ld); h == H and w == W copies bit for bit.  F16, variant 0: what the network launches (the four-pixel kernel
 *   bilinear_ac_up4x4_kernel, a 4 x 4 output block per thread, when W % 4 == 0, 3 (w-1)/(W-1) < 1, W >= 4 * (256 / (C/8)),
 *   H % 4 == 0 and 3 (h-1)/(H-1) < 1, unless EMP_BILINEAR_NO_UP4=1 was set when the process made its first call; else
 *   bilinear_ac_kernel); variant 1: bilinear_ac_kernel; variant 2: the four-pixel kernel, EMP_ERR_INVALID where those
 *   conditions fail.  EMP_BILINEAR_UP4_LEGACY=1 (read per call): the four-pixel kernel is bilinear_ac_up4_kernel (1 x 4 outputs
 *   per thread) under the first three conditions alone.  All three kernels give the same bits.  F32: variant must be 0; bilinear32x4_kernel when W % 4 == 0
 *   and W >= 4 w, unless EMP_BILINEAR32_X4=0 (read per call), else bilinear32_kernel; same bits.
 * emp_op_bilinear_ac_nchw_f32: NC planes (h,w) fp32 -> (h*scale, w*scale), align_corners=True (bilinear_ac_f32_kernel).
 * emp_op_avgpool: mean over the HW pixels of each of C channels of (N,HW,in_ld) -> d_out (N,C) fp32.  F16:
 *   avgpool_partial_kernel + avgpool_final_kernel (C % 8) with d_work of emp_op_avgpool_work_bytes bytes, which needs no
 *   initialisation; F32: avgpool32_kernel, no scratch (d_work may be NULL); HL32: avgpool_hl32_kernel on a map made by
 *   emp_hl32_from_f32 (C, in_ld % 32; rows of 2 * in_ld halfs), no scratch.
 * emp_op_gemv: out[n][co] = act(sum_k in[n][k] * w[co][k] (+ b[co] when d_b is not NULL)), fp32, act = ReLU when relu != 0
 *   (gemv_kernel: one wave per output).
 * emp_op_gate_mul: x * sigmoid(g) per element of `rows` rows of C channels.  F16 (gate_mul_f16_kernel): the result replaces g,
 *   x is left alone; F32 (gate_mul32_kernel): the result replaces x, g is left alone.
 * emp_op_dwconv_nhwc_f32: KxK (3 | 5) depthwise conv, stride 1, pad K/2, no bias, taps (K*K, C) fp32: dwconv32_strip_kernel
 *   when W % 8 == 0 unless EMP_DW32_STRIP=0 (read per call), else dwconv32_kernel; same bits. */
typedef enum { EMP_OP_F16 = 0, EMP_OP_F32 = 1, EMP_OP_HL32 = 2 } emp_op_prec;
EMP_API int emp_op_stem7x7(const void* d_img, int image_dtype, float sub, float mul, int N, int H, int W, int vh, int vw,
                           const float* d_w, const float* d_b, void* d_out, int prec, void* stream);
EMP_API int emp_op_stem_pool(const void* d_img, int image_dtype, float sub, float mul, int N, int H, int W, int vh, int vw,
                             const float* d_w, const float* d_b, void* d_out, int prec, void* stream);
EMP_API int emp_op_stem3x3s2(const void* d_img, int image_dtype, float sub, float mul, int N, int H, int W, int vh, int vw,
                             const float* d_w, const float* d_b, int C, void* d_out, int out_ld, int prec, void* stream);
EMP_API int emp_op_maxpool3x3s2(const void* d_in, int N, int H, int W, int C, void* d_out, int prec, void* stream);
EMP_API int emp_op_fuse_combine(const void* d_a, const void* d_b, const void* d_c, float ca, float cb, float cc, int mode, int N,
                                int H, int W, int C, void* d_out, void* d_out_lo, int out_ld, int prec, void* stream);
EMP_API int emp_op_bilinear_ac_nhwc(const void* d_in, int N, int h, int w, int C, int in_ld, void* d_out, int H, int W, int out_ld,
                                    int prec, int variant, void* stream);
EMP_API int emp_op_bilinear_ac_nchw_f32(const float* d_in, int NC, int h, int w, float* d_out, int scale, void* stream);
EMP_API int emp_op_avgpool_work_bytes(int N, int C, int prec, size_t* h_bytes);
EMP_API int emp_op_avgpool(const void* d_in, int N, int HW, int C, int in_ld, float* d_out, void* d_work, size_t work_bytes,
                           int prec, void* stream);
EMP_API int emp_op_gemv(const float* d_in, int N, int K, const float* d_w, const float* d_b, int Cout, int relu, float* d_out,
                        void* stream);
EMP_API int emp_op_gate_mul(void* d_x, int x_ld, void* d_g, int g_ld, int64_t rows, int C, int prec, void* stream);
EMP_API int emp_op_dwconv_nhwc_f32(const float* d_in, int N, int H, int W, int C, int in_ld, const float* d_w, int K, float* d_out,
                                   int out_ld, void* stream);

/* ------------------------------------------------------------------------
 * 3. Instance post-processing (hot loop 2), one launch group per batch
 * ---------------------------------------------------------------------- */

/* logits -> probabilities: sigmoid (C==1) or channel softmax (C>1).
 * replaces logits_to_prob, engines.py:22-30.  (N,C,H,W) fp32 in/out. */
EMP_API int emp_logits_to_prob(const float* d_logits, float* d_prob, int N, int C, int H, int W, void* stream);

/* Recursive per-pixel median over a ks-deep queue of probability maps.
 * replaces _MedianQueue.get_median, engines.py:59-66 (torch.cat + torch.median).
 * d_slices: array of ks device pointers (host array), each (C,H,W) fp32;
 * d_out may alias d_slices[mid] (that is what the reference does, :76-84). */
EMP_API int emp_median_slices(const float* const* h_slice_ptrs, int ks, float* d_out,
                      size_t count, void* stream);

/* The same filter over a run of consecutive slices in one launch (batched 3-D path): the recursion of
 * _MedianQueue.get_next (engines.py:76-84) is per pixel, so one thread carries the filtered history.
 *   d_hist (mid,count) filtered maps preceding the run; d_raw (n_raw,count) raw maps of the run plus
 *   mid look-ahead maps; d_out (n_out,count): out[j] = median(filtered[j-mid..j-1], raw[j..j+mid]).
 *   ks odd, 3..15 (the widget offers up to 11, _volume_inference.py:388).  d_out may be d_raw (in place). */
EMP_API int emp_median_recursive(const float* d_hist, const float* d_raw, int n_raw, int ks, int n_out,
                         float* d_out, size_t count, void* stream);

/* Centre NMS + voting + nearest upsampling: get_instance_cells,
 * engines.py:257-275 (find_instance_center postprocess.py:38-76 and
 * group_pixels :78-169).  Batched over N images.
 *   d_ctr_hmp (N,1,h,w) fp32, d_offsets (N,2,h,w) fp32
 *   step: 4 (coarse boundaries) or 1;  up = upsampling*step (nearest factor)
 *   d_cells (N, h*up, w*up) int32: 0 where the image has no centre
 *   d_centers (N, max_centers, 2) int32 (y,x) in row-major order,
 *   d_num_centers (N) int32 (clamped to max_centers; overflow is reported by
 *   a negative return of emp_instance_cells_check).
 *   d_work: scratch of emp_instance_cells_work_bytes(N,h,w) bytes (the NMS bit mask + a per-image grid over the centres).
 * Round 6: an image with 192 .. 16 384 centres is voted through a uniform grid over its centres (bins of ~2+ centres, rings of bins
 * searched outwards from the voted position until the next ring cannot hold a centre at the best distance found) instead of the
 * scan over every centre per pixel: the scan's cells bit for bit (same fp32 expression per candidate, lowest index among the minima
 * of the rounded distance, 1e5 start value, non-finite votes -> 0) at pixels x ~tens instead of pixels x centres evaluations
 * (1024^2 tile, 4 500 centres: 1.56 -> 0.15 ms).  EMP_VOTE_GRID=0 (read per call): the scan for every image. */
EMP_API size_t emp_instance_cells_work_bytes(int N, int h, int w);
EMP_API int emp_instance_cells(const float* d_ctr_hmp, const float* d_offsets, int N, int h, int w,
                       float nms_threshold, int nms_kernel, int step, int up,
                       int32_t* d_cells, int32_t* d_centers, int32_t* d_num_centers,
                       int max_centers, void* d_work, void* stream);

/* harden + thing-mask + majority vote + per-class renumbering + stuff filter:
 * PanopticDeepLabRenderEngine.postprocess, engines.py:277-298 with
 * merge_semantic_and_instance, postprocess.py:223-296.  Batched over N.
 *   d_sem (N,C,H,W) fp32 probabilities; d_cells (N,H,W) int32
 *   thing_list: host array of n_things class ids
 *   d_pan (N,H,W) int64 (reference dtype) ; max_ids: upper bound on cell ids
 *   d_work: scratch of emp_panoptic_merge_work_bytes(N, C, max_ids) bytes
 * The two streaming kernels move 16 bytes per lane when H * W is a multiple of 4 and d_sem, d_cells and d_pan are 16-byte
 * aligned, and one pixel per lane otherwise; EMP_MERGE_SCALAR=1 (read per call) takes the latter everywhere.  The counts
 * are integers: the result is the same either way. */
EMP_API size_t emp_panoptic_merge_work_bytes(int N, int C, int max_ids);
EMP_API int emp_panoptic_merge(const float* d_sem, const int32_t* d_cells, int N, int C, int H, int W,
                       float confidence_thr, const int32_t* h_thing_list, int n_things,
                       int64_t label_divisor, int64_t stuff_area, int64_t void_label,
                       int max_ids, int64_t* d_pan, void* d_work, void* stream);

/* ------------------------------------------------------------------------
 * 4. Label map <-> run-length encoding (3-D stitching path)
 * ---------------------------------------------------------------------- */

/* 8-connected components of EQUAL non-zero label, numbered 1..K per image in raster order of each
 * component's first pixel.  replaces rle.connected_components (skimage.measure.label / cc3d),
 * empanada/inference/rle.py:18-24, used by pan_seg_to_rle_seg (:66-69) and
 * Engine2d.force_connected (empanada_napari/inference.py:263-279).
 *   d_in, d_out (N,H,W) int32; d_num (N) int32 components per image (may be NULL). */
EMP_API size_t emp_ccl8_work_bytes(int N, int H, int W);
EMP_API int emp_ccl8(const int32_t* d_in, int N, int H, int W, int32_t* d_out, int32_t* d_num,
             void* d_work, void* stream);

/* Engine2d.force_connected, empanada_napari/inference.py:263-279, for a batch of label maps in one call: for each
 * thing class in list order, the ids in [class*divisor, (class+1)*divisor) are replaced by their 8-connected
 * components numbered in raster order + class*divisor (later classes see the earlier classes' relabelling, as the
 * reference edits pan_seg in place).  d_pan (N,H,W) int64 (the Render engine's output); d_out (N,H,W) int32 (what
 * Engine2d.infer returns after .astype(np.int32), inference.py:325); h_thing_list is a HOST array. */
EMP_API size_t emp_force_connected_work_bytes(int N, int H, int W);
EMP_API int emp_force_connected(const int64_t* d_pan, int N, int H, int W, const int32_t* h_thing_list, int n_things,
                        int64_t label_divisor, int32_t* d_out, void* d_work, void* stream);

/* 26-connected components of EQUAL non-zero label of ONE volume (skimage.measure.label on a 3-D array, default
 * full connectivity), numbered in raster order of first voxels.  replaces filters.connected_components,
 * empanada/inference/filters.py:14-20, as used by filters.pan_seg_to_rle_seg (:58-116) after erode / dilate /
 * fill_holes.  d_in, d_out (D,H,W) int32, D*H*W < 2^30; work buffer: emp_ccl8_work_bytes(1, D*H, W). */
EMP_API int emp_ccl26(const int32_t* d_in, int D, int H, int W, int32_t* d_out, int32_t* d_num,
              void* d_work, void* stream);

/* One grey erosion (op 0) / dilation (op 1) of a uint32 label volume with the 3-D cross footprint, border mode
 * 'reflect'.  replaces skimage.morphology.erosion / dilation as called by filters.erode / filters.dilate,
 * empanada/inference/filters.py:154-176 (one call per iteration; d_out != d_in). */
EMP_API int emp_morph_cross3d(const uint32_t* d_in, uint32_t* d_out, int D, int H, int W, int op, void* stream);

/* (host) filters.fill_holes_in_segmentation, empanada/inference/filters.py:178-210, on a host uint32 label volume in
 * place: per slice, per label in ascending order, the label's original bounding box is cut out of the current
 * slice and scipy.ndimage.binary_fill_holes of the cut-out (any label counts as foreground) is written back as
 * that label.  Slices run on threads. */
EMP_API int emp_fill_holes_slices(uint32_t* h_vol, int64_t D, int64_t H, int64_t W);

/* Runs of equal non-zero label over the raveled image, in raster order.  replaces
 * regionprops(...).coords -> rle_encode, rle.py:73-81 + array_utils.py:213-239.
 *   d_runs (N, max_runs, 3) int32 {start, length, label}; d_num_runs (N) int32 (un-clamped). */
EMP_API size_t emp_rle_extract_work_bytes(int N, int H, int W);
EMP_API int emp_rle_extract(const int32_t* d_labels, int N, int H, int W, int32_t* d_runs,
                    int32_t* d_num_runs, int max_runs, void* d_work, void* stream);

/* Round 6 -- emp_ccl8 / emp_ccl26 and emp_rle_extract with the class isolation folded into the kernels' reads: the labels of
 * [lo, hi) of an int32 (in_bytes 4) or int64 (in_bytes 8) panoptic map are kept, everything else reads as background --
 * pan_seg_to_rle_seg's `instance_seg[outside the class range] = 0` (empanada/inference/rle.py:46-48) and force_connected's
 * (empanada_napari/inference.py:270-272) without a select pass (and an int64 -> int32 pass) per class in front of the kernels.
 *   emp_ccl_range : depth 0: N images of H x W, 8-connected (work: emp_ccl8_work_bytes(N, H, W)); depth > 0 (N == 1): one
 *                   volume depth x H x W, 26-connected (work: emp_ccl8_work_bytes(1, depth * H, W)); d_num may be NULL
 *   emp_rle_extract_range : as emp_rle_extract; the run labels are the map's own values (hi < 2^31) */
EMP_API int emp_ccl_range(const void* d_in, int in_bytes, int N, int depth, int H, int W, int64_t lo, int64_t hi,
                        int32_t* d_out, int32_t* d_num, void* d_work, void* stream);
EMP_API int emp_rle_extract_range(const void* d_labels, int in_bytes, int N, int H, int W, int64_t lo, int64_t hi,
                        int32_t* d_runs, int32_t* d_num_runs, int max_runs, void* d_work, void* stream);

/* Connected components of an array too large for one emp_ccl_range call, slab by slab (csrc/components.hip): skimage.measure.label
 * on the whole array (full connectivity, equal value, numbered in raster order of first voxels) -- the components clear_border
 * clears (_filter_small_labels.py:45) -- from emp_ccl_range on slabs of leading-axis slices.  A slab's local ids 1..K plus the
 * number of components of all slabs before it (its base) are provisional ids 1..G; d_parent (n_parent >= G + 1 int32, entry g
 * initialised to g by the caller, entry 0 unused) is a union-find forest over them whose roots are the smallest ids of their sets.
 *
 * emp_ccl_seam: the unions across one seam.  d_prev_vals / d_prev_ids: the last slice (H, W) of the previous slab, its values and
 * its local ids; d_cur_vals / d_cur_ids: the first slice of the current slab.  in_bytes: 4 (int32) or 8 (int64) values, as
 * emp_ccl_range reads them; a voxel whose id is 0 (background, or a value outside the range the CCL kept) takes no part.  Every
 * other voxel (y, x) of the current slice is united with the in-bounds voxels (y + dy, x + dx), dy, dx in {-1, 0, 1}, of the
 * previous slice that hold the same value: parent entries base_cur + id and base_prev + id'.  H * W < 2^30; 0 <= base_prev <=
 * base_cur < n_parent < 2^31; an id that would fall outside d_parent is skipped, never written.  Does not synchronise. */
EMP_API int emp_ccl_seam(const void* d_prev_vals, const int32_t* d_prev_ids, const void* d_cur_vals, const int32_t* d_cur_ids,
                         int in_bytes, int H, int W, int64_t base_prev, int64_t base_cur, int32_t* d_parent, int64_t n_parent,
                         void* stream);
/* The final numbers of the provisional ids: d_parent[1..G] is flattened in place, its roots are ranked in id order (the flatten /
 * count / scan / rank steps of emp_ccl8 on ids instead of voxels) -> d_lut (G + 1) int32, d_lut[0] = 0 and d_lut[g] = the 1-based
 * rank of g's root; *d_count (device int32) = the number of roots.  0 <= G <= 2^31 - 2; G = 0 gives d_lut[0] = 0 and a count of 0.
 * Work buffer: emp_ccl_rank_roots_work_bytes(G) (0 for a G outside the domain).  Does not synchronise. */
EMP_API size_t emp_ccl_rank_roots_work_bytes(int64_t G);
EMP_API int emp_ccl_rank_roots(int32_t* d_parent, int64_t G, int32_t* d_lut, int32_t* d_count, void* d_work, void* stream);
/* d_out[i] = d_ids[i] ? d_lut[base + d_ids[i]] : 0 over the n voxels of a slab: local ids -> final numbers.  d_out may be d_ids.
 * 0 <= base < n_lut < 2^31, n_lut the entries of d_lut; an id that would fall outside it gives 0.  Does not synchronise. */
EMP_API int emp_ccl_lut(const int32_t* d_ids, const int32_t* d_lut, int64_t base, int64_t n_lut, int32_t* d_out, int64_t n,
                        void* stream);

/* Run list -> dense volume of elem_bytes-wide integers.  replaces numpy_fill_instances,
 * array_utils.py:754-766 (runs must not overlap: later-overwrites-earlier is not defined here). */
EMP_API int emp_rle_fill(const int64_t* d_starts, const int64_t* d_lens, const int64_t* d_vals,
                 int64_t nruns, void* d_volume, int64_t size, int elem_bytes, void* stream);

/* The same with the reference's overwrite order for overlapping objects: where runs overlap, the run with the highest
 * d_order (position of its instance in the dict) wins, as numpy_fill_instances' sequential fill does.  d_prio: scratch
 * of `size` int32, initialised by the call. */
EMP_API int emp_rle_fill_ordered(const int64_t* d_starts, const int64_t* d_lens, const int64_t* d_vals,
                 const int32_t* d_order, int64_t nruns, void* d_volume, int64_t size, int elem_bytes,
                 int32_t* d_prio, void* stream);

/* HOST: intersections of pairs of run-length objects stored CSR-style (object k owns runs
 * [h_off[k], h_off[k+1])).  replaces rle_intersection, array_utils.py:344-407. */
EMP_API int emp_rle_pair_intersections(const int64_t* h_starts, const int64_t* h_runs, const int64_t* h_off,
                               const int64_t* h_pairs, int64_t n_pairs, int64_t* h_out);
/* HOST: k-of-n vote over (n,2) ranges -> maximal ranges covered >= thr times (thr 1 = union).
 * replaces vote_by_ranges / rle_voting / join_ranges, array_utils.py:461-699. */
EMP_API int emp_ranges_vote(const int64_t* h_ranges, int64_t n, int thr, int64_t* h_out, int64_t* n_out);
/* HOST: copies n_seg segments of two parallel int64 arrays (run starts, run lengths): segment j = h_cnt[j] elements of
 * source array h_src_id[j] from element h_src_off[j] on, to h_out_* + h_out_off[j]; worker threads.  The concatenation of
 * the per-slab partial trackers into one tracker on rank 0 (empanada_napari/multigpu.py:240-252 builds that tracker by
 * feeding every slice to InstanceTracker.update in one process, tracker.py:61-100). */
EMP_API int emp_gather_segments_i64(const int64_t* const* h_src_a, const int64_t* const* h_src_b, const int32_t* h_src_id,
                            const int64_t* h_src_off, const int64_t* h_cnt, const int64_t* h_out_off, int64_t n_seg,
                            int64_t* h_out_a, int64_t* h_out_b);

/* ------------------------------------------------------------------------
 * 5. HOST: slice-to-slice matching + instance tracking of ONE class over a
 *    stack of slices.  replaces RLEMatcher / rle_matcher (matcher.py:136-326),
 *    forward_matching / backward_matching / apply_matchers (patterns.py:55-121)
 *    and InstanceTracker.update / finish (tracker.py:61-123).  The assignment on
 *    the IoU matrix stays with the caller (scipy.optimize.linear_sum_assignment,
 *    matcher.py:218):  step_begin -> [assignment] -> step_apply, per slice.
 * ---------------------------------------------------------------------- */
typedef struct emp_stack_matcher emp_stack_matcher_t;
EMP_API emp_stack_matcher_t* emp_sm_create(int64_t class_id, int64_t label_divisor, double iou_thr, double ioa_thr,
                                   int do_match);
EMP_API void emp_sm_destroy(emp_stack_matcher_t* h);
/* append a slice: (n,3) {start, length, label} runs in raster order (emp_rle_extract output), plane width, id offset */
EMP_API int emp_sm_push_slice_runs(emp_stack_matcher_t* h, const int64_t* h_runs, int64_t n, int64_t width, int64_t id_offset);
/* `count` slices at once (one launch group of the run extractor), built on the library's worker threads (EMP_SM_THREADS,
 * default 4; emp_sm_prepare uses the same threads for the pair tables) */
EMP_API int emp_sm_push_slices_runs(emp_stack_matcher_t* h, int64_t count, const int64_t* const* runs, const int64_t* n,
                                    int64_t width, int64_t id_offset);
/* append a slice as objects: labels (n), boxes (n,4), CSR offsets (n+1), starts, runs */
EMP_API int emp_sm_push_slice_objects(emp_stack_matcher_t* h, int64_t n, const int64_t* labels, const int64_t* boxes,
                              const int64_t* off, const int64_t* starts, const int64_t* runs);
EMP_API int64_t emp_sm_num_slices(const emp_stack_matcher_t* h);
/* Slab-wise matching (one matcher per rank: multigpu.py).  The forward / backward passes of patterns.py:68-121 are a chain
 * along the axis, but what a slice hands to its neighbour is small: the grouping of its components into labelled objects
 * (dict order) and RLEMatcher.next_label (matcher.py:254-268).  A rank pushes its own slab plus the neighbours' boundary
 * slices ("ghosts": same runs, hence same component indices), builds all pair tables up front with emp_sm_prepare (the
 * label-independent bulk: run intersections of neighbouring slices), imports the state of a ghost slice as its target and
 * runs emp_sm_run over its own slices only; emp_sm_track takes the GLOBAL slice position.
 *   emp_sm_prepare     : pair tables of local slices (from, to]
 *   emp_sm_state_size / emp_sm_export_state : objects of local slice idx as labels[n_obj], CSR off[n_obj+1], members[n_mem]
 *                        (component indices), and the label counter
 *   emp_sm_import_state: slice idx gets these objects and becomes the target; next_label < 0 keeps the counter;
 *                        assign_new 1 = forward pass, 0 = backward pass (patterns.py:102-109) */
/* scipy.optimize.linear_sum_assignment(cost, maximize=True), as matcher.py:218 calls it, on a dense row-major (nr, nc)
 * float64 matrix: min(nr, nc) pairs with ascending rows.  The library's own solver (scipy's shortest-augmenting-path
 * algorithm restated, ties included); emp_sm_run uses it for the assignment blocks unless EMP_SM_SCIPY=1. */
EMP_API int emp_lsa_maximize(const double* cost, int64_t nr, int64_t nc, int64_t* rows, int64_t* cols);
/* the same assignment from the matrix's non-zero entries only (er[k], ec[k]) -> ew[k] (an IoU matrix is almost all
 * zeros): the algorithm, its floating-point values and its tie-breaking are those of the dense form, the per-step scan of
 * all columns is replaced by a segment tree -- what the slice matcher calls (csrc/matcher.hip lsa_maximize_sparse) */
EMP_API int emp_lsa_maximize_sparse(int64_t nr, int64_t nc, int64_t nnz, const int64_t* er, const int64_t* ec, const double* ew,
                                    int64_t* rows, int64_t* cols);
EMP_API int emp_sm_prepare(emp_stack_matcher_t* h, int64_t from, int64_t to);
EMP_API int emp_sm_state_size(const emp_stack_matcher_t* h, int64_t idx, int64_t* n_obj, int64_t* n_mem);
EMP_API int emp_sm_export_state(const emp_stack_matcher_t* h, int64_t idx, int64_t* labels, int64_t* off, int64_t* members,
                                int64_t* next_label);
EMP_API int emp_sm_import_state(emp_stack_matcher_t* h, int64_t idx, int64_t n_obj, const int64_t* labels, const int64_t* off,
                                const int64_t* members, int64_t next_label, int assign_new);
EMP_API int emp_sm_begin_backward(emp_stack_matcher_t* h);
/* First half of RLEMatcher.__call__ (matcher.py:280-326) for slice idx.  nt / nm: number of target / slice objects;
 * nt < 0: nothing to assign (target initialised / class not matched).  The overlap matrix is held sparse (candidates by a
 * 64-pixel grid over the boxes, exact run intersections); the connected components of its graph that are a single
 * (target, object) pair are assigned by the library -- any optimal assignment contains them, every other entry of their
 * row and column is 0 and zero-IoU pairs never pass the threshold (matcher.py:226-229) -- and the rest forms the SOLVER
 * BLOCK: emp_sm_pending_shape gives its shape (0 x 0: nothing to solve), emp_sm_iou its dense float64 IoU matrix (rows /
 * columns in ascending original order).  The caller runs scipy.optimize.linear_sum_assignment(maximize=True) on the block,
 * as the reference does on the whole matrix (matcher.py:218), and passes the result, in BLOCK coordinates, to
 * emp_sm_step_apply (n = 0 when the block is empty). */
EMP_API int emp_sm_step_begin(emp_stack_matcher_t* h, int64_t idx, int* nt, int* nm);
EMP_API const double* emp_sm_iou(const emp_stack_matcher_t* h);          /* solver block, valid until the next step */
EMP_API int emp_sm_step_apply(emp_stack_matcher_t* h, const int64_t* rows, const int64_t* cols, int64_t n);
/* Runs `count` steps from slice idx in direction dir (+1 / -1), feeding the tracker after each when `track`, and stops
 * before the first slice with a non-empty solver block (*stopped_at = its index, step pending: solve emp_sm_iou with
 * linear_sum_assignment, emp_sm_step_apply, emp_sm_track, resume), or runs to the end (*stopped_at = -1).
 * Replaces the per-slice Python loop of forward_matching / backward_matching, patterns.py:68-121. */
EMP_API int emp_sm_run(emp_stack_matcher_t* h, int64_t idx, int dir, int64_t count, int track, int64_t* stopped_at);
/* shape of the pending step's solver block */
/* steps with competing overlaps solved so far by the sparse solver (default) / by a dense solver call on the IoU matrix
 * (EMP_SM_FULL_LSA=1 the whole matrix as the reference hands it to scipy, empanada/inference/matcher.py:216-218; =0 the conflict block) */
EMP_API int emp_sm_solver_stats(const emp_stack_matcher_t* h, int64_t* sparse_steps, int64_t* dense_steps);
EMP_API int emp_sm_pending_shape(const emp_stack_matcher_t* h, int* nt, int* nm);
EMP_API int emp_sm_tracker_init(emp_stack_matcher_t* h, int axis /* 0 xy, 1 xz, 2 yz */, int64_t D, int64_t H, int64_t W);
EMP_API int emp_sm_track(emp_stack_matcher_t* h, int64_t idx, int64_t index2d);
/* InstanceTracker.update over local slices last, last-1, ..., first at positions global_first + (i - first) (the order
 * backward_matching feeds the tracker: empanada/inference/patterns.py:102-134, tracker.py:61-97), every track sized once. */
EMP_API int emp_sm_track_range(emp_stack_matcher_t* h, int64_t first, int64_t last, int64_t global_first);
EMP_API int emp_sm_tracker_finish(emp_stack_matcher_t* h);
EMP_API int64_t emp_sm_num_tracks(const emp_stack_matcher_t* h);
EMP_API int emp_sm_track_info(const emp_stack_matcher_t* h, int64_t k, int64_t* label, int64_t* box6, int64_t* n_runs);
EMP_API int emp_sm_track_runs(const emp_stack_matcher_t* h, int64_t k, int64_t* starts, int64_t* runs);
/* the same for ALL tracks in one call each (tracker.instances as flat arrays: labels (T), boxes (T,6), run counts (T) --
 * any of the three may be NULL -- and the run lists back to back in track order) */
EMP_API int emp_sm_tracks_info(const emp_stack_matcher_t* h, int64_t* labels, int64_t* boxes6, int64_t* counts, int64_t* total_runs);
EMP_API int emp_sm_tracks_runs(const emp_stack_matcher_t* h, int64_t* starts, int64_t* runs);
EMP_API int64_t emp_sm_slice_num_objects(const emp_stack_matcher_t* h, int64_t idx);
EMP_API int emp_sm_slice_object_info(const emp_stack_matcher_t* h, int64_t idx, int64_t k, int64_t* label, int64_t* box4,
                             int64_t* n_runs);
EMP_API int emp_sm_slice_object_runs(const emp_stack_matcher_t* h, int64_t idx, int64_t k, int64_t* starts, int64_t* runs);

/* ------------------------------------------------------------------------
 * 6. Scoring of label volumes (csrc/overlap.hip): the sparse contingency table
 *    of two label arrays on the device, and the matching derived from it.
 *    replaces the dense np.histogram2d over label VALUES + np.bincount of the
 *    plugin's model-performance tool (empanada_napari/_accuracy_metrics.py:
 *    121-131) and the per-pair rle_iou loop of the offline evaluator
 *    (empanada/inference/matcher.py:194-204 as called from
 *    empanada/evaluation/evaluator.py:88-89).
 *
 *    The table is a device buffer of emp_label_overlap_work_bytes(capacity)
 *    bytes (capacity: slots, a power of two in [64, 2^32]) that the caller
 *    resets once and then feeds slab by slab; it survives between calls.
 *    Labels must lie in [0, 2^32).  The counts are exact uint64 integers.
 * ---------------------------------------------------------------------- */
/* 0 if the capacity is not a power of two in [64, 2^32] */
EMP_API size_t emp_label_overlap_work_bytes(int64_t capacity);
EMP_API int emp_label_overlap_reset(void* d_table, int64_t capacity, void* stream);
/* Adds the n voxel pairs (d_a[i], d_b[i]) to the table: conf_matrix of _accuracy_metrics.py:125 restricted to its non-zero
 * cells, accumulated.  a_bytes / b_bytes: element size 1, 2, 4 or 8, NEGATIVE for a signed type (int32: -4), as
 * emp_ccl_range takes in_bytes.  A value outside [0, 2^32) -- negative, or 2^32 and above -- is an error (EMP_ERR_INVALID,
 * the table's content is then undefined), never wrapped.  Synchronises the stream.  *h_overflow = 1: the table is too small for
 * this slab; the call has removed what it had added (the table is as before): move the table to a larger one with
 * emp_label_overlap_grow and call again. */
EMP_API int emp_label_overlap_accumulate(const void* d_a, int a_bytes, const void* d_b, int b_bytes, int64_t n, void* d_table,
                                 int64_t capacity, void* stream, int* h_overflow);
/* Re-inserts the cells of d_from into the reset, larger table d_to.  Synchronises.  *h_overflow = 1: d_to is too small too. */
EMP_API int emp_label_overlap_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream,
                                 int* h_overflow);
/* The occupied cells as d_keys[i] = a << 32 | b and d_counts[i], in no particular order (sort the keys: the result is then
 * np.unique(a << 32 | b, return_counts=True)); *h_num = their number, of which min(*h_num, max_out) are written.
 * Synchronises.  The table stays valid and can be fed further. */
EMP_API int emp_label_overlap_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, int64_t max_out,
                                 int64_t* h_num, void* stream);
/* HOST: from the k cells (h_a[i], h_b[i]) -> h_count[i], sorted by (a, b): the non-zero labels of each side in ascending order
 * with their areas (gt_ids / gt_area / pred_ids / pred_area of _accuracy_metrics.py:96-99,130-131; target_labels /
 * match_labels of matcher.py:179-183), IoU = inter / (area_a + area_b - inter) in float64 (_accuracy_metrics.py:134-136,
 * array_utils.py:427-433) and the assignment linear_sum_assignment(-iou) == linear_sum_assignment(iou, maximize=True)
 * (_accuracy_metrics.py:145-146, matcher.py:213) through emp_lsa_maximize_sparse.  index_space 0: one row / column per label
 * that occurs (the evaluator); 1: one per integer 1..max label, the absent ones empty (the tool's histogram bins), labels up
 * to 2^26.  Out: the assigned pairs that overlap, rows ascending, as indices into the label lists, with their IoU and
 * intersection; pairs without overlap (IoU 0) are not returned.  Every output array holds k entries. */
EMP_API int emp_overlap_match(int64_t k, const int64_t* h_a, const int64_t* h_b, const int64_t* h_count, int index_space,
                      int64_t* h_a_labels, int64_t* h_a_areas, int64_t* n_a, int64_t* h_b_labels, int64_t* h_b_areas, int64_t* n_b,
                      int64_t* h_rows, int64_t* h_cols, double* h_iou, int64_t* h_inter, int64_t* n_match);

/* ------------------------------------------------------------------------
 * 7. Clean-up of label volumes (csrc/labels.hip): the per-label table (voxel
 *    count and bounding box of every label that occurs) and the edit of a
 *    volume through a `from -> to` map.  The two primitives behind the
 *    plugin's Filter Small Labels (empanada_napari/_filter_small_labels.py:
 *    15-60), Count Labels (_label_counter_widget.py:105-118, :243), Delete
 *    Labels (_merge_split_widget.py:212-280), Merge Labels (:282-420), Jump to
 *    Label (:637-680) and Find Next Available Label (:682-763).
 *
 *    skimage is not available where this library is built: what
 *    regionprops_table (area, bbox) and clear_border compute is restated from
 *    their documented behaviour and is NOT pinned against them (like rows
 *    a13 / a14 of the README table); the tests state it in numpy / scipy.
 *
 *    The table is a device buffer of emp_label_table_work_bytes(capacity)
 *    bytes with the life cycle and the overflow contract of section 6: reset
 *    once, fed slab by slab, grown when an accumulate reports an overflow.
 * ---------------------------------------------------------------------- */
/* 0 if the capacity is not a power of two in [64, 2^32] */
EMP_API size_t emp_label_table_work_bytes(int64_t capacity);
EMP_API int emp_label_table_reset(void* d_table, int64_t capacity, void* stream);
/* Adds the slab d_labels (depth, H, W) whose first leading-axis index is z0 to the table: per key the uint64 voxel count
 * (regionprops_table's `area`, _filter_small_labels.py:16; np.unique(return_counts=True)) and the min / max of z, y, x in GLOBAL
 * coordinates (regionprops' bbox, _merge_split_widget.py:653-655; the box clear_border's border test needs,
 * _filter_small_labels.py:45).  in_bytes: element size 1, 2, 4 or 8, NEGATIVE for a signed type, as emp_ccl_range and
 * emp_label_overlap_accumulate take it.  per_slice 0: key = the label, any value in [0, 2^63); per_slice 1: key =
 * slice << 32 | label with labels in [0, 2^32) (the widgets' "2D patches" mode, _filter_small_labels.py:120-125).  A value
 * outside the domain, negative included, is EMP_ERR_INVALID (the table's content is then undefined), never wrapped.  Label 0 is
 * a key like any other.  z0 + depth < 2^31.  Synchronises the stream.  *h_overflow = 1: the table is too small for this slab;
 * the call has removed the counts it had added (the min / max it left in stored keys are idempotent: they are the right values
 * once the slab is counted again): move the table to a larger one with emp_label_table_grow and call again. */
EMP_API int emp_label_table_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int per_slice,
                                 void* d_table, int64_t capacity, void* stream, int* h_overflow);
/* Re-inserts the counted cells of d_from into the reset, larger table d_to.  Synchronises.  *h_overflow = 1: d_to is too small too. */
EMP_API int emp_label_table_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream,
                                 int* h_overflow);
/* *h_num = the number of keys, of which min(*h_num, max_out) are written, in no particular order: d_keys[i], d_counts[i] and
 * d_boxes[6 i ..] = {min z, min y, min x, max z, max y, max x}, the maxima INCLUSIVE (regionprops' bbox has them exclusive: + 1).
 * Synchronises.  The table stays valid and can be fed further. */
EMP_API int emp_label_table_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint32_t* d_boxes,
                                 int64_t max_out, int64_t* h_num, void* stream);
/* An open-addressing map of n entries h_keys[i] -> h_vals[i] (HOST arrays; keys in [0, 2^63), a key given twice keeps its last
 * value) in the device arrays d_map_keys / d_map_vals of map_capacity uint64 each; map_capacity: a power of two in [64, 2^32],
 * at least 2 n.  Synchronises. */
EMP_API int emp_label_map_build(const uint64_t* h_keys, const uint64_t* h_vals, int64_t n, uint64_t* d_map_keys, uint64_t* d_map_vals,
                                 int64_t map_capacity, void* stream);
/* d_out[i] = map[key(i)] if present, else d_src[i], over the slab (depth, H, W) starting at leading-axis index z0: all
 * `labels[labels == l] = v` passes of remove_label_from_image (_filter_small_labels.py:10-12,27-28), Delete Labels
 * (_merge_split_widget.py:249-250) and Merge Labels (:385-387) in one.  key(i) = d_key[i], or slice << 32 | d_key[i] with
 * per_slice 1.  d_key may be d_src (delete, merge, filter) or another array of the same shape (component ids: only the
 * components of a label that touch a border go, as clear_border does it); d_out may be d_src.  d_out has d_src's element size.
 * A key value of 0 is background and is never looked up; a value outside the key's domain is in no map.  Does not synchronise. */
EMP_API int emp_label_apply_map(const void* d_key, int key_bytes, const void* d_src, int src_bytes, void* d_out, int64_t z0, int depth,
                                 int H, int W, int per_slice, const uint64_t* d_map_keys, const uint64_t* d_map_vals,
                                 int64_t map_capacity, void* stream);

/* ------------------------------------------------------------------------
 * 7b. Measure Labels (csrc/measure.hip): per label that occurs, background 0
 *    excepted, what regionprops_table is asked for after a segmentation:
 *    `area` (the voxel count), `bbox`, and the raw sums behind `centroid`
 *    (sum of each coordinate / area), `moments` (sum z^a y^b x^c up to order 2)
 *    and `inertia_tensor` (from the central second moments); plus the number
 *    of exposed voxel faces per axis, this library's statement of a surface
 *    (regionprops' `perimeter` is a weighted boundary-pixel count and is not
 *    reproduced).  As in section 7 skimage is not available where this
 *    library is built: everything is restated from documented behaviour and
 *    is NOT pinned against it; the tests state it in numpy / scipy.
 *
 *    The table has the life cycle and the overflow contract of sections 6 and
 *    7.  All sums are uint64 and exact.
 * ---------------------------------------------------------------------- */
/* 0 if the capacity is not a power of two in [64, 2^32] */
EMP_API size_t emp_label_measure_work_bytes(int64_t capacity);
EMP_API int emp_label_measure_reset(void* d_table, int64_t capacity, void* stream);
/* Adds the slab d_labels (depth, H, W), slices [z0, z0 + depth) of a volume of total_depth slices, to the table.  in_bytes, the
 * keys (per_slice 0: the label in [0, 2^63); 1: slice << 32 | label, labels in [0, 2^32)) and the error for values outside the
 * domain are those of emp_label_table_accumulate, except that label 0 is background and is never entered.  Per key:
 *   count          the voxels (regionprops_table's `area`)
 *   box            min / max of z, y, x in global coordinates (`bbox`)
 *   S1             sum z, sum y, sum x (`centroid` = S1 / count; `moments` of order 1)
 *   S2             sum zz, yy, xx, zy, zx, yx (`moments` of order 2; n S2 - S1 S1 are n^2 times the central moments behind
 *                  `inertia_tensor`)
 *   F              faces perpendicular to z, y, x: one per voxel of the label and direction in which the neighbour has another
 *                  value, 0 included; with border_faces != 0 also where the neighbour lies outside the array (the first and
 *                  last index of each axis; for z: slices 0 and total_depth - 1)
 * d_halo: slice z0 - 1 (H * W elements of the same type) on the device, so that z-faces across the slab's lower border are
 * counted; NULL for z0 == 0.  With per_slice 1 no z-faces are counted and d_halo is not read.  Shapes with
 * max(D, H, W)^2 * D * H * W >= 2^63 are EMP_ERR_INVALID: a raw second moment could wrap.  Synchronises the stream.
 * *h_overflow = 1: the table is too small for this slab; the call has removed what it had added (box fields are idempotent and
 * stay): move the table to a larger one with emp_label_measure_grow and call again. */
EMP_API int emp_label_measure_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                                 const void* d_halo, int per_slice, int border_faces, void* d_table, int64_t capacity, void* stream,
                                 int* h_overflow);
/* Re-inserts the counted cells of d_from into the reset, larger table d_to.  Synchronises.  *h_overflow = 1: d_to is too small too. */
EMP_API int emp_label_measure_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream,
                                 int* h_overflow);
/* *h_num = the number of keys, of which min(*h_num, max_out) are written, in no particular order: d_keys[i], d_counts[i],
 * d_boxes[6 i ..] as emp_label_table_finalize writes them (maxima INCLUSIVE), d_sums[9 i ..] = S1 then S2 in the order above,
 * d_faces[3 i ..] = F.  Synchronises.  The table stays valid and can be fed further. */
EMP_API int emp_label_measure_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint32_t* d_boxes,
                                 uint64_t* d_sums, uint64_t* d_faces, int64_t max_out, int64_t* h_num, void* stream);

/* ------------------------------------------------------------------------
 * 7c. Shape Labels (csrc/shape.hip): per label that occurs, background 0
 *    excepted, the integers behind a smooth surface and a hole count: the
 *    intercept counts along the 13 half-directions of the 26-neighbourhood
 *    (Cauchy-Crofton: surface = 2 sum_k c_k I_k v / |d_k|, with the weights
 *    c_k the host derives from the spacing; in an image the perimeter from
 *    the first four) and the Euler number under full and under face
 *    connectivity.  What skimage's perimeter_crofton and euler_number
 *    compute is restated from their documentation and is NOT pinned against
 *    them (skimage is not available where this library is built); pinned
 *    are the integers against a numpy statement and the axis intercepts
 *    against section 7b's faces.
 *
 *    The table has the life cycle and the overflow contract of sections 6,
 *    7 and 7b.  A slot is 136 bytes.  All sums are exact; the Euler sums are
 *    signed and kept modulo 2^64.
 * ---------------------------------------------------------------------- */
/* 0 if the capacity is not a power of two in [64, 2^32] */
EMP_API size_t emp_label_shape_work_bytes(int64_t capacity);
EMP_API int emp_label_shape_reset(void* d_table, int64_t capacity, void* stream);
/* Adds the slab d_labels (depth, H, W), slices [z0, z0 + depth) of a volume of total_depth slices, to the table: arguments, keys,
 * value domain, d_halo and errors are those of emp_label_measure_accumulate (there is no moment guard; total_depth < 2^31 and
 * H, W < 2^30).  Per key, with M the voxels of the label:
 *   count          the voxels
 *   I[k], k < 13   the half-directions d_k are the (dz, dy, dx) in {-1, 0, 1}^3 \ {0} whose first non-zero component is +1, in
 *                  ascending lexicographic order: (0,0,1), (0,1,-1), (0,1,0), (0,1,1), (1,-1,-1), .., (1,1,1).
 *                  I[k] = #{p in M : p + d_k not in M} + #{p in M : p - d_k not in M}.  border_faces != 0: a neighbour outside
 *                  the array is not in M; 0: a pair with one end outside the array is not counted.  I[8], I[2], I[0] are the F
 *                  of section 7b.  per_slice 1: only k < 4 (the directions of an image) are counted, the rest stay 0.
 *   chi[0]         the Euler number of the union of the closed voxel cubes of M (full connectivity: 26, in an image 8):
 *                  vertices - edges + faces - voxels of the cubical complex, on the array padded with background
 *   chi[1]         the Euler number under face connectivity (6 / 4): voxels - face pairs inside M + 2 x 2 quads inside M -
 *                  2 x 2 x 2 octets inside M.  per_slice 1: both are the image's, nothing crosses slices.
 * An image (R, W) is passed as the volume (R, 1, W): its four directions are k = 0, 7, 8, 9, and both Euler numbers are the
 * image's.  The vertices on the faces z = total_depth, y = H, x = W of the array are counted by the voxels at the last index,
 * for z by the slab that holds the last slice.  Synchronises the stream.  *h_overflow = 1 as in section 7b. */
EMP_API int emp_label_shape_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                                 const void* d_halo, int per_slice, int border_faces, void* d_table, int64_t capacity, void* stream,
                                 int* h_overflow);
/* Re-inserts the counted cells of d_from into the reset, larger table d_to.  Synchronises.  *h_overflow = 1: d_to is too small too. */
EMP_API int emp_label_shape_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow);
/* *h_num = the number of keys, of which min(*h_num, max_out) are written, in no particular order: d_keys[i], d_counts[i],
 * d_intercepts[13 i ..] = I, d_euler[2 i ..] = chi.  Synchronises.  The table stays valid and can be fed further. */
EMP_API int emp_label_shape_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint64_t* d_intercepts,
                                 int64_t* d_euler, int64_t max_out, int64_t* h_num, void* stream);

/* ------------------------------------------------------------------------
 * 7d. Contact Labels (csrc/contacts.hip): per unordered pair {a, b} of
 *    different label values that occur next to each other, the number of
 *    voxel pairs that join them along each of the 13 half-directions d_k of
 *    section 7c -- the integers behind the area two objects share and behind
 *    a region adjacency graph.  This section has no counterpart in the
 *    reference plugin; the nearest thing is skimage's region adjacency graph
 *    (skimage.graph.RAG, rag_boundary), and it is NOT pinned against skimage
 *    (not available where this library is built): the tests state the
 *    definition in numpy, and the sums over a label's partners are pinned
 *    against section 7c's intercepts and section 7b's faces.
 *
 *      N[k] = #{p : p and p + d_k both in the array, {L(p), L(p + d_k)} = {a, b}}
 *      count = sum_k N[k]; a pair exists exactly if its count is positive
 *      key = min(a, b) << 32 | max(a, b), labels in [0, 2^32)
 *
 *    A pair with an end outside the array is never counted (there is no
 *    border_faces here).  background 0: a pair with a 0 in it is not
 *    entered; != 0: it is entered under the key (0, b).  There is no
 *    per_slice: slice, a and b do not fit a 64-bit key.  Summed over the
 *    partners b of a label a, 0 included, N[k](a, b) is I[k] of a in section
 *    7c with border_faces 0.
 *
 *    The table has the life cycle and the overflow contract of sections 6,
 *    7, 7b and 7c.  A slot is 120 bytes.  Every column is exact and does not
 *    depend on the slabs.
 * ---------------------------------------------------------------------- */
/* 0 if the capacity is not a power of two in [64, 2^32] */
EMP_API size_t emp_label_contacts_work_bytes(int64_t capacity);
EMP_API int emp_label_contacts_reset(void* d_table, int64_t capacity, void* stream);
/* Adds the pairs whose later end lies in the slab d_labels (depth, H, W), slices [z0, z0 + depth) of a volume of total_depth
 * slices, to the table.  in_bytes in {1, 2, 4, 8}, negative = signed; total_depth < 2^31 and H, W < 2^30; a value outside
 * [0, 2^32) -- an 8-byte value with a high word, a negative signed value -- is EMP_ERR_INVALID ("a label outside ...") and
 * leaves the table undefined.  d_halo: slice z0 - 1 (H * W elements of the same type) on the device: the pairs across the
 * slab's lower border are counted by this, the upper, slab and by no other; NULL for z0 == 0.  An image (R, W) is passed as the
 * volume (R, 1, W): its four directions are k = 0, 7, 8, 9.  Synchronises the stream.  *h_overflow = 1 as in section 7b. */
EMP_API int emp_label_contacts_accumulate(const void* d_labels, int in_bytes, int64_t z0, int depth, int H, int W, int64_t total_depth,
                                 const void* d_halo, int background, void* d_table, int64_t capacity, void* stream, int* h_overflow);
/* Re-inserts the counted cells of d_from into the reset, larger table d_to.  Synchronises.  *h_overflow = 1: d_to is too small too. */
EMP_API int emp_label_contacts_grow(const void* d_from, int64_t from_capacity, void* d_to, int64_t to_capacity, void* stream, int* h_overflow);
/* *h_num = the number of pairs, of which min(*h_num, max_out) are written, in no particular order: d_keys[i], d_counts[i],
 * d_pairs[13 i ..] = N.  Synchronises.  The table stays valid and can be fed further. */
EMP_API int emp_label_contacts_finalize(void* d_table, int64_t capacity, uint64_t* d_keys, uint64_t* d_counts, uint64_t* d_pairs /* 13 per row */,
                                 int64_t max_out, int64_t* h_num, void* stream);

/* ------------------------------------------------------------------------
 * 8. Morph Labels (csrc/morph.hip): binary dilation, erosion, closing and
 *    opening of single labels with a disk / ball of radius 1..7, every label
 *    inside its own padded box -- the plugin's Morph Labels
 *    (empanada_napari/_merge_split_widget.py:46-209); its fifth operation,
 *    `Fill holes` (remove_small_holes inside the same padded box), is
 *    emp_fill_holes_labels at the end of this section.
 *
 *    skimage is not available where this library is built: binary_dilation
 *    and binary_erosion are restated from their documented behaviour
 *    (scipy.ndimage.binary_dilation(structure=footprint) and
 *    scipy.ndimage.binary_erosion(structure=footprint, border_value=True);
 *    disk / ball = x^2 + y^2 (+ z^2) <= r^2) and are NOT pinned against
 *    skimage; the tests state the loop with scipy.
 * ---------------------------------------------------------------------- */
/* the ops of the widget's table (_merge_split_widget.py:48-53) */
#define EMP_MORPH_DILATE 0
#define EMP_MORPH_ERODE 1
#define EMP_MORPH_CLOSE 2 /* erode(dilate) */
#define EMP_MORPH_OPEN 3  /* dilate(erode) */
/* The core (cz, cy, cx) of the tiles emp_morph_labels works on: cx = 64 - 2 * radius * stages (a mask row with its halo is one
 * 64-bit word; stages: 2 for Close and Open), (cz, cy) = (1, 64) for the disk and (8, 16) for the ball (ball != 0,
 * _merge_split_widget.py:92-95). */
EMP_API int emp_morph_tile_shape(int radius, int ball, int op, int* cz, int* cy, int* cx);
/* The loop over label_ids of _merge_split_widget.py:123-134, IN PLACE on d_vol (D, H, W; a 2-D image is D = 1, ball = 0;
 * elem_bytes as in section 7), by levels: the turns (one label each) of a level must touch disjoint parts of the array -- their
 * boxes, padded by the radius, do not intersect -- and levels run in order, so that the result is the sequential loop's.
 *   d_turn_labels[t]   the label of turn t
 *   d_turn_boxes[6 t]  {min z, y, x, max z, y, x} (inclusive) of the label when its turn comes: given for the turns of the first
 *                      level (regionprops' bbox, :125); for later levels initialised to {2^32 - 1 x 3, 0 x 3} and computed here
 *                      from the array as it is then.  A label without a voxel left is skipped (the reference raises an
 *                      IndexError there, `[...][0]` of an empty list, :125).
 *   d_tiles[4 i]       {turn, z0, y0, x0}: the first voxel of a tile's core; the cores of a turn's tiles are disjoint and cover
 *                      the largest padded box (_pad_box, :56-67) the turn can have; level l owns the tiles
 *                      [h_level_offsets[l], h_level_offsets[l + 1])
 *   d_scratch          scratch_words uint64: cz * cy per tile of the largest level
 * Per level: the boxes (not for the first level), the new masks into the scratch buffer (`binary = op(crop == label_id)`,
 * :130-133; outside the crop is false for a dilation and true for an erosion), then the edit (`crop[binary_before] = 0`,
 * `crop[binary] = label_id`, :132,134).  *h_launches = the number of kernel launches.  Does not synchronise. */
EMP_API int emp_morph_labels(void* d_vol, int elem_bytes, int D, int H, int W, int radius, int ball, int op,
                             const uint64_t* d_turn_labels, uint32_t* d_turn_boxes, int64_t n_turns, const int32_t* d_tiles,
                             const int64_t* h_level_offsets, int n_levels, uint64_t* d_scratch, int64_t scratch_words, void* stream,
                             int* h_launches);

/* The core (cz, cy, cx) of the tiles emp_fill_holes_labels works on: (1, 64, 64) for an image and (8, 16, 64) for a volume
 * (ball != 0); there is no halo. */
EMP_API int emp_fill_holes_tile_shape(int ball, int* cz, int* cy, int* cx);
/* The same loop with operation == 'Fill holes' (_merge_split_widget.py:53,90-91,123-134), IN PLACE on d_vol:
 * `binary = remove_small_holes(crop == label_id, hole_size)`, `crop[binary] = label_id`, where crop is the label's box as the
 * array is then, padded by the radius and clipped (the radius applies to every operation, :56-67; ball: pad along z as well).
 * The complement of the mask INSIDE THE CROP is split into its components of connectivity 1 (4 neighbours in an image, 6 in a
 * volume, no diagonals), and every voxel of a component with fewer than hole_size voxels (`<`) becomes the label, whatever it
 * held; a component that touches the crop's border is a component like any other.  hole_size <= 1 changes nothing (no launch).
 * Levels, d_turn_labels, d_turn_boxes, d_tiles (cores of emp_fill_holes_tile_shape) and h_level_offsets as in emp_morph_labels;
 * the turns of a level write inside their padded boxes, so the levels are those of a dilation.
 *   d_turn_frames[7 t]  {z0, y0, x0, nz, ny, nx, offset}: the box the host padded, clipped and covered with tiles for turn t --
 *                       it holds the turn's crop -- and the turn's first entry in d_parent / d_size; a voxel's entry is offset +
 *                       its linear position in the frame.  The frames of a level do not share entries; levels reuse them.
 *   d_parent, d_size    scratch_entries int32 each (< 2^31 - 1): the voxels of the frames of the largest level
 * Per level: the boxes (not for the first level), the parents of the background voxels, the unions with the x - 1, y - 1 and
 * z - 1 neighbours (lock-free union-find, the root is the smallest entry), the component sizes (integer atomics: the result is
 * bit-reproducible), then the edit.  *h_launches = the number of kernel launches.  Does not synchronise.
 * remove_small_holes / remove_small_objects are restated from their source and are NOT pinned against skimage. */
EMP_API int emp_fill_holes_labels(void* d_vol, int elem_bytes, int D, int H, int W, int radius, int ball, int64_t hole_size,
                                  const uint64_t* d_turn_labels, uint32_t* d_turn_boxes, const int64_t* d_turn_frames,
                                  int64_t n_turns, const int32_t* d_tiles, const int64_t* h_level_offsets, int n_levels,
                                  int32_t* d_parent, int32_t* d_size, int64_t scratch_entries, void* stream, int* h_launches);

/* ------------------------------------------------------------------------
 * 9. Split Labels (csrc/split.hip): the device side of the plugin's Split
 *    Labels (empanada_napari/_merge_split_widget.py:422-634) -- distance
 *    transform, peak candidates, the marker flood and the write-back, batched
 *    over the boxes of all turns of a call.  The greedy spacing of the peaks,
 *    ndi.label of the survivors and the id bookkeeping (:527-545) are the
 *    host's (labels.py, split_labels).
 *
 *    A box is 8 int64 {z0, y0, x0, nz, ny, nx, offset, label}: the label's
 *    TIGHT box (regionprops' bbox, :519; an image is D = 1, nz = 1) and the
 *    box's first entry in every per-voxel array; a voxel's entry is offset +
 *    its raster position in the box, and the boxes follow each other without
 *    gaps.  Every entry takes the boxes from the HOST (h_boxes), checks them
 *    -- inside the array, nz^2 + ny^2 + nx^2 < 2^30, at most 65535 boxes,
 *    n_entries < 2^31 - 1 -- and uploads them to d_boxes (8 n_boxes int64).
 *
 *    Pinned against scipy, exactly: the distance transform and the maximum
 *    filter.  Restated from memory and NOT pinned (skimage is not available
 *    where this library is built): peak_local_max's predicate, and the
 *    flood's order, which is the level-synchronous form below and not
 *    skimage's sequential queue.
 * ---------------------------------------------------------------------- */
/* what a voxel carries whose row / plane / box holds no background */
#define EMP_SPLIT_INF (1 << 30)
/* d_work of emp_split_edt: three int32 arrays of n_entries */
EMP_API size_t emp_split_edt_work_bytes(int64_t n_entries);
/* `ndi.distance_transform_edt(crop == label)` (_merge_split_widget.py:429), SQUARED and exact: d_d2[entry] = the squared
 * Euclidean distance (int32) to the nearest voxel of the CROP that is not the label; voxels outside the crop are not
 * background.  A row scan, then per remaining axis the lower envelope of parabolas.  A box without any background is
 * EMP_SPLIT_INF everywhere (scipy returns an artefact there; the caller treats such a label as "nothing to split").
 * d_vol (D, H, W; elem_bytes as in section 7) is only read.  Does not synchronise. */
EMP_API int emp_split_edt(const void* d_vol, int elem_bytes, int D, int H, int W, const int64_t* h_boxes, int n_boxes, int64_t* d_boxes,
                          int32_t* d_d2, int64_t n_entries, void* d_work, void* stream);
EMP_API size_t emp_split_peaks_work_bytes(int64_t n_entries, int n_boxes);
/* The candidates of `peak_local_max(distance, min_distance=d)` (_merge_split_widget.py:435,442) before its spacing rule, from
 * any int32 image per box (d_d2): a voxel with value == the maximum of the (2d + 1)^n window around it clamped to the box
 * (ndi.maximum_filter(size=2d + 1, mode='nearest')), value > the box's minimum (threshold_abs = image.min()), and not within d
 * voxels of either end of an axis (exclude_border=True); axes of length 1 take no part (the squeeze of :434-440).  A constant
 * box has no candidate.  d = min_distance in 1..100 (the widget's slider, :461).
 *   d_cand[3 i]      {box, raster position in the box, value} in raster order, box after box; only the first cand_capacity
 *                    are written
 *   d_box_counts[b]  the number of candidates of box b, written or not: their sum says whether the capacity was enough
 * Does not synchronise the results (it synchronises once on its own upload). */
EMP_API int emp_split_peaks(const int64_t* h_boxes, int n_boxes, int64_t* d_boxes, int D, int H, int W, const int32_t* d_d2,
                            int64_t n_entries, int min_distance, int32_t* d_cand, int64_t cand_capacity, int32_t* d_box_counts,
                            void* d_work, void* stream);
EMP_API size_t emp_split_flood_work_bytes(int64_t n_entries, int64_t n_markers);
/* `watershed(energy, markers, mask=binary)` (_merge_split_widget.py:530) in its level-synchronous form.  The mask is d_d2 > 0;
 * the energy is -d_d2 (plateau == 0, distance mode, :430) or constant (plateau != 0, points mode, :455).
 *   every mask voxel gets a time (L, g) and a label; a marker voxel has time (e, 0) and its marker's id; any other voxel q takes
 *   the label of the face neighbour p in the mask (4 in an image, 6 in a volume) with the lexicographically smallest
 *   (L_p, g_p, label_p), and the time (L_p, g_p + 1) if e(q) <= L_p, else (e(q), 0).
 * Times strictly increase along a claim chain, so the solution is unique; it is found by recomputing every voxel from its
 * neighbours' values of the sweep before until a sweep changes nothing (no atomic minimum: a stale label with an equal time would
 * stick).  skimage's flood is a sequential priority queue over (value, age): on one plateau (points mode) the two agree on
 * every voxel; in distance mode a few per cent of a label's voxels, next to the border between two regions, can differ.
 *   h_markers[3 i]  {box, raster position in the box, id}, id in 1..2^30 - 1 (host memory); one on a voxel outside the mask is ignored
 *   d_out[entry]    the id that claimed the voxel; 0 outside the mask and in a part of the mask no marker reaches
 *   *h_sweeps       the number of sweeps, the last one, which changed nothing, included
 * Synchronises: the change flags come back every 8 sweeps. */
EMP_API int emp_split_flood(const int64_t* h_boxes, int n_boxes, int64_t* d_boxes, int D, int H, int W, const int32_t* d_d2,
                            int64_t n_entries, int plateau, const int32_t* h_markers, int64_t n_markers, int32_t* d_out, void* d_work,
                            void* stream, int64_t* h_sweeps);
/* `labels[slices][binary] = new_labels[binary] + max_label` (_merge_split_widget.py:544), IN PLACE on d_vol: every voxel of box b
 * that holds the box's label becomes d_bases[b] + d_markers[entry] (so a voxel that no marker reached becomes d_bases[b], as in
 * the reference).  d_bases[b] < 0: the turn writes nothing ("nothing to split", or the ids are in use, :540-542).  The new ids
 * must not occur in the array and must fit the element type: the host's bookkeeping sees to both.  Does not synchronise. */
EMP_API int emp_split_write(void* d_vol, int elem_bytes, int D, int H, int W, const int64_t* h_boxes, int n_boxes, int64_t* d_boxes,
                            const int32_t* d_markers, int64_t n_entries, const int64_t* d_bases, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMPANADA_HIP_H */
