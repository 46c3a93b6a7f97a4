// What the two halves of the network scheduler share: pdl_net.hip (parameter list, packers, arena plan, the fp16 schedule,
// the C entries) and pdl_net32.hip (the fp32 / fp16x3 graph).
#pragma once

#include <string.h>

#include <array>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"

namespace emp {

struct HostParam {
  std::vector<int64_t> shape;
  std::vector<float> w, b;
  bool set = false;
};

struct Act {  // NHWC fp16 activation
  half_t* p = nullptr;
  int N = 0, H = 0, W = 0, C = 0, ld = 0;
  size_t off = 0;
};

struct DevConv {  // packed conv weights
  half_t* w = nullptr;
  half_t* w256 = nullptr;         // the 256 x 256 tile's image of w (conv256_pack_weights), made at the first launch that takes that tile
  float* b = nullptr;
  int cout = 0, cin = 0, cin_pad = 0, kh = 1, kw = 1;
  int cin2 = 0, cin2_pad = 0;     // K-concatenated second source (conv3 + projection shortcut)
  bool wsplit = false;            // the "second source" is the SAME input again, against the lo halves of an fp16 hi + lo weight pair
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- the topology, written once: every walk over the encoder (parameter list, packers, arena plan, both schedules) reads these ----
const int kLayers[4] = {3, 4, 6, 3};
const int kPlanes[4] = {64, 128, 256, 512};
const char* const kDecoders[2] = {"semantic_decoder", "instance_decoder"};
const char* const kHeads[3] = {"semantic_head", "ins_center", "ins_xy"};
const char* const kBifpn[2] = {"semantic", "instance"};      // "<kBifpn>_fpn", "<kBifpn>_decoder"

// ResNet50 bottleneck b of layer li (resnet.py:217-229): "encoder.layer<li>.<b>"
struct ResBlock {
  int li, b, stride, dil, planes;      // stride: of this block's conv2 and shortcut (the layer's at b == 0, else 1); dil: the layer's
  bool last;                           // last block of its layer: its output is a pyramid level
  std::string name, next;              // next: the block that follows (the next layer's first one included), empty after the last
};

inline std::vector<ResBlock> resnet_blocks(const emp_pdl_config& c) {
  std::vector<ResBlock> v;
  for (int li = 1; li <= 4; ++li) {
    int stride = li == 1 ? 1 : 2, dil = 1;
    if (li == 4 && c.stage4_stride == 16) { stride = 1; dil = 2; }
    for (int b = 0; b < kLayers[li - 1]; ++b)
      v.push_back({li, b, b == 0 ? stride : 1, dil, kPlanes[li - 1], b + 1 == kLayers[li - 1],
                   "encoder.layer" + std::to_string(li) + "." + std::to_string(b), ""});
  }
  for (size_t i = 0; i + 1 < v.size(); ++i) v[i].next = v[i + 1].name;
  return v;
}

// RegNet block b (1-based) of stage si (1-based) (regnet.py:51-97): "encoder.stage<si>.block<b>"
struct RegBlock {
  int si, b, stride, width, groups;
  bool shortcut;      // the block carries a shortcut convolution
  bool last;          // last block of its stage: its output is a pyramid level
  std::string name;
};

inline std::vector<RegBlock> regnet_blocks(const emp_pdl_config& c) {
  std::vector<RegBlock> v;
  for (int si = 1; si <= 4; ++si)
    for (int b = 1; b <= c.rn_depths[si - 1]; ++b) {
      const int w_in = si == 1 ? c.rn_stem : c.rn_widths[si - 2];
      v.push_back({si, b, b == 1 ? c.rn_strides[si - 1] : 1, c.rn_widths[si - 1], c.rn_groups[si - 1],
                   b == 1 && (w_in != c.rn_widths[si - 1] || c.rn_strides[si - 1] > 1), b == c.rn_depths[si - 1],
                   "encoder.stage" + std::to_string(si) + ".block" + std::to_string(b)});
    }
  return v;
}

}  // namespace emp

using namespace emp;

struct emp_pdl {
  emp_pdl_config cfg;
  int aspp_ch = 256, dec_ch = 256, ncls = 1;
  std::vector<ResBlock> res_blocks;      // the encoder's blocks in order (emp_pdl_create): one of the two lists is empty
  std::vector<RegBlock> reg_blocks;
  std::vector<std::string> param_names;
  std::map<std::string, HostParam> params;
  bool finalized = false;
  FILE* layer_log = [] { const char* e = getenv("EMP_LAYER_LOG"); return e ? fopen(e, "w") : (FILE*)nullptr; }();
  // fused separable convs (sepconv.hip); EMP_FUSE_SEPCONV=0 keeps the dwconv + 1x1 conv + head1x1 launches (A/B runs)
  bool fuse_stem = env_on("EMP_FUSE_STEM");   // stem.hip
  bool fuse_ds = env_on("EMP_FUSE_DS");       // conv3 + downsample in one GEMM
  bool fuse_b2b = env_on("EMP_FUSE_B2B");     // conv3 + the next block's conv1
  bool pack256 = env_on("EMP_CONV256_PACK");   // packed weight images for the 256 x 256 tile (A/B runs: 0)
  bool fuse_proj = env_on("EMP_FUSE_PROJ");   // low-level projections + the next stage's conv1
  bool fuse_aspp = env_on("EMP_FUSE_ASPP");   // the two decoders' ASPP branches as one conv each
  bool fuse_sepconv = env_on("EMP_FUSE_SEPCONV");
  bool fuse_pr = env_on("EMP_FUSE_PR");             // pointrend.hip
  // Separable blocks with an exact depthwise half (sepconv_precise.hip: fp32 taps, depthwise result as fp16 hi + lo, 2
  // MFMAs per product).  EMP_PRECISE_SEPCONV:
  //   1 (default) = the blocks the CENTRE heat-map and the offsets depend on: the last-stage fusion conv(s) of the decoder
  //                 that feeds ins_center, the ins_center head and -- BiFPN networks, round 4 -- the ins_xy head and every
  //                 3x3 node of the FPN that feeds that decoder.  The precise nodes ALWAYS run fused (no tile-count threshold): one kernel,
  //                 one rounding sequence at every batch size, so a tile's result does not depend on the batch it
  //                 arrives in;
  //   2 = every fused block and node; 0 = none (round-2 numerics);
  //   A/B switches: 3 = the ins_center head only, 4 = the decoder's fusion convs only, 5 = 1 + the nodes of BOTH FPNs,
  //   6 = 1 + the ins_xy head, 7 = round 3's default (head + fusion convs, no nodes).
  int precise_sepconv = env_int("EMP_PRECISE_SEPCONV", 1);
  // BiFPN networks (round 4): the weights of the layers the centre heat-map is most sensitive to as fp16 hi + lo PAIRS --
  // the pointwise convs of the precise 128-cout blocks (a third MFMA per product, sepconv_precise.hip WS) and the
  // transposed convs of the decoder that feeds the centre head (the lo halves ride as a K-concatenated "second source"
  // on the same input: ConvParams::in2).  tools/error_budget.py --arch bifpn: those roundings are 80 % of the weight-side
  // variance; 512^2 tile, ctr rms / scale 1.13e-3 -> 0.96e-3.  EMP_PRECISE_WSPLIT=0 switches it off (A/B).
  bool precise_wsplit = env_on("EMP_PRECISE_WSPLIT");
  // ... and the FUSED MAPS of those nodes (the fast-normalised sum a node's separable conv reads) as fp16 hi + lo pairs too:
  // fuse_combine writes channels [hi | lo] of a 2F-wide buffer and the node runs with 2F input channels, duplicated
  // depthwise taps and pointwise weights (depthwise and pointwise are linear: dw(hi) W + dw(lo) W = dw(hi + lo) W).  The
  // 24 fused-map roundings of an FPN were worth more than their share of the variance: 512^2 tile, ctr rms / scale
  // 0.96e-3 -> 0.78e-3 (format-emulating oracle).  EMP_PRECISE_FSPLIT=0 switches it off (A/B).
  bool precise_fsplit = env_on("EMP_PRECISE_FSPLIT");
  // BiFPN nodes run fused once the map has this many 8 x 16 tiles (a tile per CU); EMP_SEPCONV_MIN_TILES for A/B runs
  int sepconv_min_tiles = env_int("EMP_SEPCONV_MIN_TILES", 256);

  // fp32 reference mode (emp_pdl_set_precision / EMP_PRECISION=fp32; run32 in pdl_net32.hip): fp32 weights, fp32 activation pool
  // precision 2 = the fp16x3 mode (round 5): the fp32 mode's graph, maps and weights, its convolutions on the fp16 matrix
  // pipe with split operands (conv16x3.hip: three MFMAs per product into an fp32 accumulator)
  // Round 6: the DEFAULT is 2 -- the mode that meets the north star's tolerance (1e-3 of the reference's fp32 forward in the
  // max norm) on every network; the fp16 engine (0) is the explicit throughput opt-in (emp_pdl_set_precision(net, 0) /
  // EMP_PRECISION=fp16: ~5e-3 in the max norm)
  int precision = [] {
    const char* e = getenv("EMP_PRECISION");
    if (e && (!strcmp(e, "fp16") || !strcmp(e, "16"))) return 0;
    if (e && (!strcmp(e, "fp32") || !strcmp(e, "32"))) return 1;
    return 2;
  }();
  bool fp32_graph() const { return precision != 0; }
  // RegNet on the fp16 engine: the grouped 3x3 as ONE launch (blockIdx.y = group, conv_igemm_grouped.hip); EMP_REGNET_GROUPED=0:
  // one launch per group with its couts padded to 64 / 128 for the register-weight kernels (round 4; A/B)
  // fp16x3 mode: the heads' 1x1 fused into the pointwise conv (EMP_X3_FUSE_HEAD=0: the separate head1x1_32 launch; A/B)
  bool x3_fuse_ds = env_on("EMP_X3_FUSE_DS");      // conv3 + projection shortcut as one K-concatenated conv (A/B)
  bool x3_fuse_head = env_on("EMP_X3_FUSE_HEAD");
  // fp16x3 mode, round 6: the stride-16 region of a ResNet50 network (layer3, layer4, ASPP) as hl32 maps on conv16x3p_kernel's
  // 256 x 256 tile once a layer3 map has this many pixel tiles (one tile of 256 couts per pixel tile is a whole launch of the
  // 256-channel layers of layer3; the ASPP branches of the two decoders run merged, 512 couts per launch.  Whole step, planes vs
  // round 5's kernels: batch 4 (64 tiles) 413.8 vs 439.2 tiles/s, batch 8 (128) 520.1 vs 469.7, batch 16 545.3 vs 472.0;
  // profiles/r06_x3p.txt).
  // EMP_X3_PLANES=0: never (A/B); EMP_X3_PLANES_MIN_TILES=n
  bool x3_planes = env_on("EMP_X3_PLANES");
  int x3_planes_min_tiles = env_int("EMP_X3_PLANES_MIN_TILES", 128);
  bool x3_planes_ready = false;      // set by finalize32: every layer of the region has its packed image
  // fp16x3 mode, round 6 (late): split-K for the long-K launches that fill less than half the chip (ONE 1024^2 tile: each 3x3 ASPP branch
  // is 64 workgroups over K = 18 432) -- Conv32::kpart; EMP_X3_KSPLIT=0: never (A/B)
  bool x3_ksplit = env_on("EMP_X3_KSPLIT");
  float* x3_kpart = nullptr;      // X3_KPART_BYTES of scratch, made by finalize32
  bool x3_small_aspp = env_on("EMP_X3_SMALL_ASPP");      // below the plane region's threshold the ASPP branches still run merged on the plane kernel, K-split (A/B)
  bool x3_fuse_stem = env_on("EMP_X3_FUSE_STEM");      // stem + max-pool as one MFMA launch (A/B)
  bool x3_merge_proj = env_on("EMP_X3_MERGE_PROJ");      // both decoders' low-level projections as one launch (A/B)
  bool x3_merge_aspp = env_on("EMP_X3_MERGE_ASPP");      // both decoders' ASPP branches as one launch (A/B)
  // fp16x3 mode, round 6: a separable block (depthwise KxK -> pointwise -> act [-> head 1x1]) as ONE launch (sepconv_x3.hip) once
  // the map has this many 8 x 16 tiles (a persistent workgroup per CU); EMP_X3_FUSE_SEP=0: the depthwise launch + conv16x3 (A/B)
  bool x3_fuse_sep = env_on("EMP_X3_FUSE_SEP");
  int x3_sep_min_tiles = env_int("EMP_X3_SEP_MIN_TILES", 1);      // (256 until finding 75: fewer launches win at every size measured)
  struct SepX3 { float* dw = nullptr; half_t* pw = nullptr; int C = 0, Cout = 0, ks = 0; };
  std::map<std::string, SepX3> sepx3;      // by the block's name ("... .sepconv" without the .0 / .1)
  bool regnet_grouped = env_on("EMP_REGNET_GROUPED");
  int64_t regnet_group_tiles = env_i64("EMP_REGNET_GROUP_TILES", 2048ll);
  struct W32 { float* w = nullptr; float* b = nullptr; int cout = 0, cin = 0, cin16 = 0, kh = 1, kw = 1; uint32_t* wp = nullptr; int cin2 = 0, cin2_16 = 0; half_t* wimg = nullptr; half_t* wimgp = nullptr; int x3p_kg = 0; };
  std::map<std::string, W32> w32;
  std::map<std::string, std::pair<float*, size_t>> pool32;      // name -> (device buffer, floats)
  std::map<std::string, std::array<int, 4>> geom32;             // zero-tailed RegNet maps: the geometry a buffer was last cleared for
  // every buffer the LAST forward of the fp32 / fp16x3 graph made, in the order made (emp_pdl_map32; run32 clears it).  kind says how
  // N, H, W, C, ld are to be read: "map" NHWC rows of ld floats (fmt 1: hl32 rows, ld in channels); the others as include/empanada_hip.h lists them
  struct Map32 { std::string name, kind; float* p = nullptr; int64_t N = 0, H = 0, W = 0, C = 0, ld = 0; int fmt = 0; };
  std::vector<Map32> maps32;
  std::map<std::string, size_t> maps32_at;      // name -> its place in maps32

  // device parameters
  std::map<std::string, DevConv> convs;
  std::map<std::string, float*> f32w;  // fp32 device blobs (stem, gemv, heads)
  std::map<std::string, half_t*> f16w;  // fp16 device blobs (depthwise taps)
  std::map<std::string, std::vector<float>> fusew;  // BiFPN fast-fusion weights after relu / (sum + eps)
  std::vector<void*> owned;

  // arena
  char* arena = nullptr;
  size_t arena_cap = 0, arena_used = 0;
  int pN = 0, pH = 0, pW = 0, pRS = 0;  // planned shape (pN: the batch of the current forward)
  int capN = 0;                         // batch the arena layout was planned for (pN <= capN)
  std::map<std::string, Act> acts;
  std::vector<std::string> act_order;
  std::map<std::string, std::pair<size_t, size_t>> raw;  // name -> (offset, bytes)
  double flops = 0.0;
  // live timing of the dominant kernel class (256x256 conv tile): HIP event pairs on the launch stream, summed by
  // emp_pdl_profile_read (bench.py's roofline block)
  size_t image_bytes = 0;      // packed 256 x 256 weight images made at finalize (fp16 engine)
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  double prof_flops = 0.0;
  // The two decoders (+ their heads) are independent after the encoder: for small problems, whose launches leave CUs
  // idle (one 1024^2 tile: <= 256 workgroups per launch), the instance side runs on a second stream -- batch-1 call
  // 2.10 -> 1.85 ms, 4 tiles 4.70 -> 3.83 ms.  EMP_PAR_DECODERS = pixel count N*H*W up to which this is done (0 = never).
  // At the bench size it would still buy 1.7 % (24.74 -> 24.34 ms per 32 tiles) but time-slices CUs between launches of
  // the two streams, so that per-kernel durations (and the roofline of the dominant kernel: 0.45 -> 0.30) stop
  // describing the kernels: large problems stay on one stream.
  int64_t par_limit = env_i64("EMP_PAR_DECODERS", (int64_t)4 << 20);
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  ~emp_pdl() {
    for (void* p : owned) (void)hipFree(p);
    for (auto& kv : pool32) (void)hipFree(kv.second.first);
    if (arena) (void)hipFree(arena);
    if (layer_log) fclose(layer_log);
    for (auto& e : prof_events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (aux) (void)hipStreamDestroy(aux);
  }
};

namespace emp {

inline int head_planes(const emp_pdl* n, int k) { return k == 0 ? n->ncls : k; }      // output planes of kHeads[k]: ncls, 1, 2

enum { ACT_NONE, ACT_RELU, ACT_SILU };      // ConvParams::act / Conv32::act

// defined in pdl_net.hip
int dev_upload(emp_pdl* n, const void* h, size_t bytes, void** out);
int upload_heads_f32(emp_pdl* n);
void split_aspp_project(const HostParam& hp, int A, HostParam* head, std::vector<float>* tail);
std::vector<float> padded_predictor(const HostParam& hp, int ncls, int ldp);
int upload_f32(emp_pdl* n, const std::string& key, const std::vector<float>& v);
int upload_regnet_stem(emp_pdl* n);
// defined in pdl_net32.hip
int finalize32(emp_pdl* n);
int run32(emp_pdl* n, const void* img, int dtype, float sub, float mul, int N, int H, int W, int vh, int vw, int RS, int interp,
          float* o_sem, float* o_ctr, float* o_off, hipStream_t s);

}  // namespace emp

#define RC(x)            \
  do {                   \
    int _rc = (x);       \
    if (_rc) return _rc; \
  } while (0)

// emp_pdl_profile: one launch between a pair of HIP events on its stream (emp_pdl_profile_read sums them), booked at `flops`
template <typename Launch>
int profiled_launch(emp_pdl* n, hipStream_t s, double flops, Launch launch) {
  if (n->prof_used == n->prof_events.size()) {
    hipEvent_t a, b;
    EMP_CHECK_HIP(hipEventCreate(&a));
    EMP_CHECK_HIP(hipEventCreate(&b));
    n->prof_events.emplace_back(a, b);
  }
  auto& ev = n->prof_events[n->prof_used++];
  EMP_CHECK_HIP(hipEventRecord(ev.first, s));
  const int rc = launch();
  EMP_CHECK_HIP(hipEventRecord(ev.second, s));
  n->prof_flops += flops;
  return rc;
}

// One forward's arguments and what the stages of either schedule hand on: the pyramid's maps (index 0: the stem / p1 map), the
// decoders' outputs and the heads' buffers, by name
struct Forward {
  emp_pdl* n;
  const emp_pdl_config& c;
  const void* img;
  int dtype;
  float sub, mul;
  int N, H, W, vh, vw, RS, interp;
  float *o_sem, *o_ctr, *o_off;
  hipStream_t s;
  std::string pyr[5], dec_out[2];
  float* head_out[3] = {nullptr, nullptr, nullptr};
};

// device memory the network owns (freed with it), uninitialised: count elements of T
template <typename T>
int dev_alloc(emp_pdl* n, size_t count, T** out) {
  void* d = nullptr;
  EMP_CHECK_HIP(hipMalloc(&d, count * sizeof(T)));
  n->owned.push_back(d);
  *out = (T*)d;
  return EMP_OK;
}

// conv3 and the projection shortcut of a bottleneck as one weight matrix [Cout][cin3 | cin_ds], either K range padded to a multiple
// of `pad` channels, with the summed (folded BN) bias: relu(conv3(c2) + downsample(x)) becomes a single GEMM over the concatenated
// K (ConvParams::in2 / Conv32::in2).  T: half_t (fp16 engine) or float (fp16x3 mode)
template <typename T>
int concat_conv3_ds(emp_pdl* n, const std::string& block, int pad, int* cout, int* cin, int* cin_pad, int* cin2, int* cin2_pad,
                    std::vector<T>* pk, std::vector<float>* b) {
  const HostParam& h3 = n->params.at(block + ".conv3");
  const HostParam& hd = n->params.at(block + ".downsample.0");
  EMP_REQUIRE(h3.shape.size() == 4 && hd.shape.size() == 4 && h3.shape[0] == hd.shape[0] && h3.shape[2] == 1 &&
                  hd.shape[2] == 1 && h3.b.size() == hd.b.size(), "%s: conv3 / downsample shapes do not match", block.c_str());
  *cout = (int)h3.shape[0];
  *cin = (int)h3.shape[1];
  *cin_pad = round_up(*cin, pad);
  *cin2 = (int)hd.shape[1];
  *cin2_pad = round_up(*cin2, pad);
  const size_t K = (size_t)*cin_pad + *cin2_pad;
  pk->assign((size_t)*cout * K, (T)0.f);
  b->resize((size_t)*cout);
  for (int o = 0; o < *cout; ++o) {
    for (int i = 0; i < *cin; ++i) (*pk)[o * K + i] = (T)h3.w[(size_t)o * *cin + i];
    for (int i = 0; i < *cin2; ++i) (*pk)[o * K + *cin_pad + i] = (T)hd.w[(size_t)o * *cin2 + i];
    (*b)[o] = h3.b[o] + hd.b[o];
  }
  return EMP_OK;
}

// An extern "C" entry's body: no exception (a map's .at() on a name two walks disagree on, bad_alloc) crosses the boundary
template <typename Body>
int guarded(const char* entry, Body body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", entry);
    return EMP_ERR_NOMEM;
  } catch (const std::exception& e) {
    set_error("%s: %s", entry, e.what());
    return EMP_ERR_STATE;
  }
}

// One BiFPN layer (bifpn.py:47-69, 103-137), shared by both schedules: top-down P7 -> P3, then bottom-up P3' -> P7, on the maps
// feat[lv] (level index lv: 0 = P3 .. 4 = P7), which leave as the layer's outputs.  pre: the layer's parameter prefix, L: its maps'.
//   resample(rk, src, dst, &name): if the resampling conv rk exists, run it from map src into map dst; name = the map to read
//   node(dirpre, q, a, b, c, ca, cb, cc, mode, out): ca * a + cb * b [+ cc * c; c may be empty] and the node's separable block into
//   map out (mode 1: a bottom-up node)
template <typename Resample, typename Node>
int bifpn_layer(const emp_pdl* n, const std::string& pre, const std::string& L, std::string feat[5], Resample resample, Node node) {
  std::string newfeat[5];
  for (int up = 0; up < 2; ++up) {
    const std::string dp = pre + (up ? ".bottom_up_fpn" : ".top_down_fpn");
    const float* w = n->fusew.at(dp + ".weights").data();
    std::string prev = up ? L + ".P3.td" : feat[4];
    if (up) newfeat[0] = prev;
    for (int i = 0; i < 4; ++i) {
      const int lv = up ? i + 1 : 3 - i;
      const std::string q = L + ".P" + std::to_string(3 + lv), out = q + (up ? ".bu" : ".td");
      std::string in;
      RC(resample(dp + ".resamplings." + std::to_string(i) + ".conv.0", feat[lv], q + (up ? ".rbu" : ".rtd"), &in));
      if (up && i < 3) {
        const float den = w[i] + w[i + 1] + w[i + 2] + 1e-4f;
        RC(node(dp, q, prev, in, q + ".td", w[i] / den, w[i + 1] / den, w[i + 2] / den, 1, out));
      } else {
        const float den = w[i] + w[i + 1] + 1e-4f;
        RC(node(dp, q, prev, in, std::string(), w[i] / den, w[i + 1] / den, 0.f, up, out));
      }
      prev = out;
      if (up) newfeat[lv] = prev;
    }
  }
  for (int lv = 0; lv < 5; ++lv) feat[lv] = newfeat[lv];
  return EMP_OK;
}
