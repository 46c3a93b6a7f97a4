// Panoptic-DeepLab + PointRend forward on gfx950: the layer schedule of
// QuantizablePanopticDeepLabPR.forward (eval) over the HIP kernels of this
// library.  Reference: empanada/models/quantization/panoptic_deeplab.py:103-115,
// 194-250; encoders/resnet.py:217-229; decoders/panoptic_deeplab.py:68-80;
// decoders/aspp.py:96-102; heads.py:12-19; point_rend.py:241-269.
//
// Data layout in HBM: activations NHWC fp16 in one arena (no aliasing: every
// intermediate stays addressable for the parity taps), conv weights fp16
// [Cout][KH*KW][Cin padded to 64], biases fp32, head outputs fp32 NCHW.
// Algebraic restructurings (all exact in real arithmetic):
//  * BatchNorm folded into the preceding conv by the host (weights.py);
//  * the ASPP image-pooling branch is a per-image constant after its 1x1 conv,
//    so it enters the 5-branch projection as a per-image bias instead of a
//    broadcast + concat (decoders/aspp.py:45-48,99-102);
//  * torch.cat is free: producers write into channel slices of one buffer;
//  * the unused first semantic_head call of _encode_decode (:107) is skipped.
#include "pdl_net.h"

namespace emp {      // shared with pdl_net32.hip (declared in pdl_net.h)

int dev_upload(emp_pdl* n, const void* h, size_t bytes, void** out) {
  void* d = nullptr;
  EMP_CHECK_HIP(hipMalloc(&d, bytes ? bytes : 16));
  n->owned.push_back(d);
  if (bytes) EMP_CHECK_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  *out = d;
  return EMP_OK;
}

int upload_f32(emp_pdl* n, const std::string& key, const std::vector<float>& v) {
  return dev_upload(n, v.data(), v.size() * sizeof(float), (void**)&n->f32w[key]);
}

// RegNet stem (W,1,3,3) -> [9][W] fp32 (both precisions compute it in fp32)
int upload_regnet_stem(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  const HostParam& hp = n->params["encoder.stem.cbr.0"];
  EMP_REQUIRE(hp.shape.size() == 4 && hp.shape[0] == c.rn_stem && hp.shape[1] == 1 && hp.shape[2] == 3 && hp.shape[3] == 3,
              "encoder.stem.cbr.0 must be (%d,1,3,3)", c.rn_stem);
  std::vector<float> w((size_t)9 * c.rn_stem);
  for (int o = 0; o < c.rn_stem; ++o)
    for (int t = 0; t < 9; ++t) w[(size_t)t * c.rn_stem + o] = hp.w[(size_t)o * 9 + t];
  RC(upload_f32(n, "rn.stem.w", w));
  return upload_f32(n, "rn.stem.b", hp.b);
}

// the heads' 1x1 weights and the PointRend predictor's bias: fp32 in every mode
int upload_heads_f32(emp_pdl* n) {
  for (int k = 0; k < 3; ++k) {
    const std::string p = kHeads[k];
    RC(upload_f32(n, p + ".head.1.w", n->params[p + ".head.1"].w));
    RC(upload_f32(n, p + ".head.1.b", n->params[p + ".head.1"].b));
  }
  return upload_f32(n, "pr.predictor.b", n->params["semantic_pr.point_head.predictor"].b);
}

// aspp.project.0 (A, 5A, 1, 1): its first 4A input channels as a conv of the concat buffer (head, with the bias), the pooled
// branch's last A as the matrix of the per-image bias GEMV (tail, row-major (A, A))
void split_aspp_project(const HostParam& hp, int A, HostParam* head, std::vector<float>* tail) {
  head->shape = {A, 4 * A, 1, 1};
  head->w.resize((size_t)A * 4 * A);
  head->b = hp.b;
  head->set = true;
  tail->resize((size_t)A * A);
  for (int o = 0; o < A; ++o) {
    for (int i = 0; i < 4 * A; ++i) head->w[(size_t)o * 4 * A + i] = hp.w[(size_t)o * 5 * A + i];
    for (int i = 0; i < A; ++i) (*tail)[(size_t)o * A + i] = hp.w[(size_t)o * 5 * A + 4 * A + i];
  }
}

// the PointRend predictor's (ncls, K) weight with its rows zero-padded to the point rows' width ldp
std::vector<float> padded_predictor(const HostParam& hp, int ncls, int ldp) {
  const int K = (int)hp.shape[1];
  std::vector<float> w((size_t)ncls * ldp, 0.f);
  for (int o = 0; o < ncls; ++o)
    for (int i = 0; i < K; ++i) w[(size_t)o * ldp + i] = hp.w[(size_t)o * K + i];
  return w;
}

}  // namespace emp

namespace {

// does the separable block `pre` (its parameters are pre.sepconv.0 / pre.sepconv.1) run with the exact depthwise half (sepconv_precise.hip)?
bool precise_layer(const emp_pdl* n, const std::string& pre) {
  const int mode = n->precise_sepconv;
  if (mode <= 0) return false;
  if (mode == 2) return true;
  const char* dec = n->cfg.ins_decoder ? "instance_decoder." : "semantic_decoder.";
  const bool head = pre.compare(0, 11, "ins_center.") == 0, fuse = pre.compare(0, strlen(dec), dec) == 0;
  if (mode == 3) return head;      // A/B switches: only the head / only the decoder's fusion convs
  if (mode == 4) return fuse;
  // the offsets head: mode 6, and by default on BiFPN networks (there the offsets sat at 1.1e-3 of their scale with it in
  // fp16 and the block is a 128-channel one: +0.5 % of a forward; the Panoptic-DeepLab offsets are at 7e-4 without it)
  if ((mode == 6 || (mode == 1 && n->cfg.arch == 1)) && pre.compare(0, 7, "ins_xy.") == 0) return true;
  return head || fuse;
}

// does the 3x3 separable node block of the BiFPN whose parameter names start with `name` ("semantic_fpn..." /
// "instance_fpn...") run with the exact depthwise half?  Default: the FPN that feeds the centre / offset heads.
bool precise_node(const emp_pdl* n, const std::string& name) {
  const int mode = n->precise_sepconv;
  if (mode == 2 || mode == 5) return true;
  if (mode != 1 && mode != 6) return false;
  const char* fp = n->cfg.ins_decoder ? "instance_fpn." : "semantic_fpn.";
  return name.compare(0, strlen(fp), fp) == 0;
}

// hi + lo weight pairs (emp_pdl::precise_wsplit): BiFPN networks, the modes with precise nodes
bool wsplit_on(const emp_pdl* n) {
  const int mode = n->precise_sepconv;
  return n->cfg.arch == 1 && n->precise_wsplit && (mode == 1 || mode == 2 || mode == 5 || mode == 6);
}

// the fused maps of this FPN's nodes travel as hi + lo pairs (emp_pdl::precise_fsplit): name starts with "<dec>_fpn."
bool fsplit_on(const emp_pdl* n, const std::string& name) {
  const int F = n->cfg.fpn_dim;
  return wsplit_on(n) && n->precise_fsplit && n->fuse_sepconv && precise_node(n, name) && sepconvp_supported(2 * F, F, 0);
}

void expect(emp_pdl* n, const std::string& name) {
  n->param_names.push_back(name);
  n->params[name] = HostParam();
}

void expect_bifpn(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  expect(n, "p2_resample.conv.0");
  const int F = c.fpn_dim;
  const bool rn = c.encoder == 1;
  const int w0[5] = {rn ? c.rn_widths[1] : 512, rn ? c.rn_widths[2] : 1024, rn ? c.rn_widths[3] : 2048, F, F};
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    std::string fp = std::string(kBifpn[d]) + "_fpn";
    expect(n, fp + ".p6_resample.conv.0");
    for (int li = 0; li < c.fpn_layers; ++li) {
      int nins[5];
      for (int i = 0; i < 5; ++i) nins[i] = li == 0 ? w0[i] : F;
      const int td[4] = {nins[3], nins[2], nins[1], nins[0]};
      const int bu[4] = {nins[1], nins[2], nins[3], nins[4]};
      for (int dir = 0; dir < 2; ++dir) {
        std::string pre = fp + ".bifpns." + std::to_string(li) + (dir == 0 ? ".top_down_fpn" : ".bottom_up_fpn");
        for (int i = 0; i < 4; ++i)
          if ((dir == 0 ? td[i] : bu[i]) != F) expect(n, pre + ".resamplings." + std::to_string(i) + ".conv.0");
        expect(n, pre + ".after_combines.0.0.sepconv.0");
        expect(n, pre + ".after_combines.0.0.sepconv.1");
        expect(n, pre + ".weights");
      }
    }
    std::string dp = std::string(kBifpn[d]) + "_decoder";
    for (int i = 0; i < 5; ++i) expect(n, dp + ".upsamplings." + std::to_string(i) + ".0");
    expect(n, dp + ".fusion.0.sepconv.0");
    expect(n, dp + ".fusion.0.sepconv.1");
  }
}

void build_param_list(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  if (c.encoder == 1) {
    expect(n, "encoder.stem.cbr.0");
    for (const RegBlock& k : n->reg_blocks) {
      const std::string& p = k.name;
      expect(n, p + ".bottleneck.a.0");
      expect(n, p + ".bottleneck.b.0");
      if (c.rn_se) {
        expect(n, p + ".bottleneck.se.se.0");
        expect(n, p + ".bottleneck.se.se.2");
      }
      expect(n, p + ".bottleneck.c.0");
      if (k.shortcut) expect(n, p + ".downsample.conv.0");
    }
  } else {
    expect(n, "encoder.conv1");
    for (const ResBlock& k : n->res_blocks) {
      const std::string& p = k.name;
      expect(n, p + ".conv1");
      expect(n, p + ".conv2");
      expect(n, p + ".conv3");
      if (k.b == 0) expect(n, p + ".downsample.0");
    }
  }
  if (c.arch == 1) expect_bifpn(n);
  for (int d = 0; d < ((c.arch == 0 && c.ins_decoder) ? 2 : (c.arch == 0 ? 1 : 0)); ++d) {
    std::string p = kDecoders[d];
    expect(n, p + ".aspp.convs.0.0");
    for (int i = 1; i <= 3; ++i) expect(n, p + ".aspp.convs." + std::to_string(i) + ".0");
    expect(n, p + ".aspp.convs.4.aspp_pooling.1");
    expect(n, p + ".aspp.project.0");
    for (int i = 0; i < c.n_stages; ++i) expect(n, p + ".project." + std::to_string(i) + ".0");
    for (int i = 0; i < c.n_stages; ++i) {
      expect(n, p + ".fuse." + std::to_string(i) + ".0.sepconv.0");
      expect(n, p + ".fuse." + std::to_string(i) + ".0.sepconv.1");
    }
  }
  for (int h = 0; h < 3; ++h) {
    std::string p = kHeads[h];
    expect(n, p + ".head.0.0.sepconv.0");
    expect(n, p + ".head.0.0.sepconv.1");
    expect(n, p + ".head.1");
  }
  for (int k = 0; k < c.num_fc; ++k) expect(n, "semantic_pr.point_head.fc_layers." + std::to_string(k) + ".0");
  expect(n, "semantic_pr.point_head.predictor");
}

// packed weights and bias to the device, the conv under its name
int store_conv(emp_pdl* n, const std::string& name, DevConv dc, const std::vector<half_t>& pk, const std::vector<float>& b) {
  RC(dev_upload(n, pk.data(), pk.size() * sizeof(half_t), (void**)&dc.w));
  RC(dev_upload(n, b.data(), b.size() * sizeof(float), (void**)&dc.b));
  n->convs[name] = dc;
  return EMP_OK;
}

// OIHW fp32 -> [O][KH*KW][Ipad] fp16 (+ fp32 bias); src: pack this parameter under `name` instead of params[name]
int pack_conv(emp_pdl* n, const std::string& name, int cin_pad_to = 0, const HostParam* src = nullptr) {
  const HostParam& hp = src ? *src : n->params.at(name);
  EMP_REQUIRE(hp.shape.size() == 4 || hp.shape.size() == 3, "%s: conv weight must be 3-d or 4-d", name.c_str());
  DevConv dc;
  dc.cout = (int)hp.shape[0];
  dc.cin = (int)hp.shape[1];
  dc.kh = hp.shape.size() == 4 ? (int)hp.shape[2] : 1;
  dc.kw = hp.shape.size() == 4 ? (int)hp.shape[3] : 1;
  dc.cin_pad = cin_pad_to ? cin_pad_to : round_up(dc.cin, 64);
  EMP_REQUIRE(dc.cin_pad >= dc.cin, "%s: bad padding", name.c_str());
  const int kt = dc.kh * dc.kw;
  std::vector<half_t> pk((size_t)dc.cout * kt * dc.cin_pad, (half_t)0.f);
  for (int o = 0; o < dc.cout; ++o)
    for (int i = 0; i < dc.cin; ++i)
      for (int t = 0; t < kt; ++t)
        pk[((size_t)o * kt + t) * dc.cin_pad + i] = (half_t)hp.w[((size_t)o * dc.cin + i) * kt + t];
  return store_conv(n, name, dc, pk, hp.b);
}

// conv3 and the projection shortcut of a bottleneck as one weight matrix [Cout][cin3_pad | cin_ds_pad] with the summed
// (folded BN) bias: relu(conv3(c2) + downsample(x)) becomes a single GEMM over the concatenated K (ConvParams::in2)
int pack_conv3_ds(emp_pdl* n, const std::string& block) {
  DevConv dc;
  std::vector<half_t> pk;
  std::vector<float> b;
  RC(concat_conv3_ds(n, block, 64, &dc.cout, &dc.cin, &dc.cin_pad, &dc.cin2, &dc.cin2_pad, &pk, &b));
  return store_conv(n, block + ".conv3+ds", dc, pk, b);
}

// fragment-ordered copy of a pointwise weight for the fused separable conv (sepconv.hip), when its shape qualifies
int pack_sepconv_pw(emp_pdl* n, const std::string& name) {
  const DevConv& dc = n->convs.at(name);
  if (dc.kh != 1 || dc.kw != 1 || !sepconv5_supported(dc.cin_pad, dc.cout, 0)) return EMP_OK;
  half_t* d = nullptr;
  RC(dev_alloc(n, (size_t)dc.cin_pad * dc.cout, &d));
  RC(launch_sepconv5_pack_pw(dc.w, dc.cin_pad, dc.cin_pad, dc.cout, d, nullptr));
  EMP_CHECK_HIP(hipStreamSynchronize(nullptr));
  n->f16w[name + ".packed"] = d;
  return EMP_OK;
}

// fragment-ordered fp16 copy of a pointwise weight for the fused separable conv with the exact depthwise half
// (sepconv_precise.hip), when its shape qualifies
// dup: the weight rows twice, [W | W] -- for an input that arrives as channels [hi | lo] (fsplit_on)
int pack_sepconvp_pw(emp_pdl* n, const std::string& name, bool dup = false) {
  const DevConv& dc = n->convs.at(name);
  const int cin_eff = (dup ? 2 : 1) * dc.cin_pad;
  if (dc.kh != 1 || dc.kw != 1 || !sepconvp_supported(cin_eff, dc.cout, 0)) return EMP_OK;
  const HostParam& hp = n->params.at(name);
  std::vector<float> w32((size_t)dc.cout * cin_eff, 0.f);
  for (int o = 0; o < dc.cout; ++o)
    for (int i = 0; i < dc.cin; ++i) {
      w32[(size_t)o * cin_eff + i] = hp.w[(size_t)o * dc.cin + i];
      if (dup) w32[(size_t)o * cin_eff + dc.cin_pad + i] = hp.w[(size_t)o * dc.cin + i];
    }
  void* tmp = nullptr;
  EMP_CHECK_HIP(hipMalloc(&tmp, w32.size() * sizeof(float)));
  hipError_t e = hipMemcpy(tmp, w32.data(), w32.size() * sizeof(float), hipMemcpyHostToDevice);
  void* d = nullptr;
  const bool ws = wsplit_on(n) && sepconvp_wsplit_supported(dc.cout);
  if (e == hipSuccess) e = hipMalloc(&d, (size_t)(ws ? 2 : 1) * cin_eff * dc.cout * sizeof(half_t));
  if (e != hipSuccess) {
    (void)hipFree(tmp);
    set_error("%s: packing the pointwise weights: %s", name.c_str(), hipGetErrorString(e));
    return EMP_ERR_HIP;
  }
  n->owned.push_back(d);
  int rc = launch_sepconvp_pack_pw((const float*)tmp, cin_eff, cin_eff, dc.cout, (half_t*)d, nullptr, ws ? 1 : 0);
  n->convs[name].wsplit = ws;
  e = hipStreamSynchronize(nullptr);
  (void)hipFree(tmp);
  if (rc) return rc;
  EMP_CHECK_HIP(e);
  n->f16w[name + (dup ? ".packedpd" : ".packedp")] = (half_t*)d;
  return EMP_OK;
}

// depthwise (C,1,5,5) -> [25][Cpad] fp16
int pack_dw(emp_pdl* n, const std::string& name, int cpad, bool dup = false) {
  const HostParam& hp = n->params.at(name);
  const int C = (int)hp.shape[0];
  EMP_REQUIRE(hp.shape.size() == 4 && hp.shape[1] == 1 && hp.shape[2] == hp.shape[3] &&
                  (hp.shape[2] == 5 || hp.shape[2] == 3) && cpad >= C,
              "%s: expected a (C,1,k,k) depthwise weight with k in {3,5}", name.c_str());
  EMP_REQUIRE(cpad % 64 == 0, "%s: padded channel count must be a multiple of 64", name.c_str());
  const int KK = (int)(hp.shape[2] * hp.shape[3]);
  std::vector<half_t> pk((size_t)KK * cpad, (half_t)0.f);
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < KK; ++t) pk[(size_t)t * cpad + c] = (half_t)hp.w[(size_t)c * KK + t];
  RC(dev_upload(n, pk.data(), pk.size() * sizeof(half_t), (void**)&n->f16w[name]));
  // the fp32-accurate fused separable conv (sepconv_precise.hip) keeps the taps in fp32 (they only meet the fp32 vector pipe), chunk-major
  // [cpad/64][KK][64]: the order of launch_sepconvp_pack_dw
  std::vector<float> pk32((size_t)KK * cpad, 0.f);
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < KK; ++t) pk32[((size_t)(c >> 6) * KK + t) * 64 + (c & 63)] = hp.w[(size_t)c * KK + t];
  if (dup) {      // the same taps for channels [0, cpad) and [cpad, 2 cpad): the input arrives as [hi | lo] (fsplit_on)
    std::vector<float> d2((size_t)2 * KK * cpad, 0.f);
    std::copy(pk32.begin(), pk32.end(), d2.begin());
    std::copy(pk32.begin(), pk32.end(), d2.begin() + (size_t)KK * cpad);
    RC(upload_f32(n, name + ".f32d", d2));
  }
  return upload_f32(n, name + ".f32", pk32);
}

// ConvTranspose2d(k=2,s=2) weight (Cin,Cout,2,2) -> 1x1 conv with 4*Cout outputs [(dy*2+dx)*Cout + co][Cin]
// split: rows [hi | lo] -- the fp16 residuals of the weights behind them, multiplied with the same input as a
// K-concatenated second source (ConvParams::in2 = in): w*x = hi*x + lo*x in one fp32 accumulation
int pack_convT(emp_pdl* n, const std::string& name, bool split = false) {
  const HostParam& hp = n->params.at(name);
  EMP_REQUIRE(hp.shape.size() == 4 && hp.shape[2] == 2 && hp.shape[3] == 2, "%s: expected (Cin,Cout,2,2)", name.c_str());
  DevConv dc;
  dc.cin = (int)hp.shape[0];
  const int co = (int)hp.shape[1];
  dc.cout = 4 * co;
  dc.cin_pad = round_up(dc.cin, 64);
  dc.kh = dc.kw = 1;
  if (split) { dc.cin2 = dc.cin; dc.cin2_pad = dc.cin_pad; dc.wsplit = true; }
  const size_t K = (size_t)dc.cin_pad + dc.cin2_pad;
  std::vector<half_t> pk((size_t)dc.cout * K, (half_t)0.f);
  std::vector<float> b((size_t)dc.cout, 0.f);
  for (int q = 0; q < 4; ++q)
    for (int o = 0; o < co; ++o) {
      b[(size_t)q * co + o] = hp.b[o];
      for (int i = 0; i < dc.cin; ++i) {
        const float w = hp.w[(((size_t)i * co + o) * 2 + (q >> 1)) * 2 + (q & 1)];
        const half_t hi = (half_t)w;
        pk[((size_t)q * co + o) * K + i] = hi;
        if (split) pk[((size_t)q * co + o) * K + dc.cin_pad + i] = (half_t)(w - (float)hi);
      }
    }
  return store_conv(n, name, dc, pk, b);
}

// BiFPN fast-fusion weights of a node group: relu(w) / (sum + eps) on the host (bifpn.py:52-55)
int set_fusew(emp_pdl* n, const std::string& nm) {
  const HostParam& hp = n->params[nm];
  EMP_REQUIRE(hp.w.size() == 5, "%s: expected 5 fusion weights", nm.c_str());
  std::vector<float> w(5);
  float sum = 0.f;
  for (int i = 0; i < 5; ++i) { w[i] = hp.w[i] > 0.f ? hp.w[i] : 0.f; sum += w[i]; }
  for (int i = 0; i < 5; ++i) w[i] = w[i] / (sum + 1e-4f);
  n->fusew[nm] = w;
  return EMP_OK;
}

// ---- arena planning ------------------------------------------------------
struct Planner {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

void add_act(emp_pdl* n, Planner& pl, const std::string& name, int N, int H, int W, int C, int ld = 0) {
  Act a;
  a.N = N; a.H = H; a.W = W; a.C = C; a.ld = ld ? ld : C;
  a.off = pl.take((size_t)N * H * W * a.ld * sizeof(half_t));
  n->acts[name] = a;
  n->act_order.push_back(name);
}
void add_raw(emp_pdl* n, Planner& pl, const std::string& name, size_t bytes) {
  n->raw[name] = {pl.take(bytes), bytes};
}

// what the stages of plan() share: the batch, the pyramid's level sizes (index 0: the stem / p1 map) and the heads' resolution
struct Plan {
  emp_pdl* n;
  Planner pl;
  int N, H, W, RS;
  int ph[5], pw[5];
  int hq = 0, wq = 0;
  void act(const std::string& name, int h, int w, int C, int ld = 0) { add_act(n, pl, name, N, h, w, C, ld); }
  void raw(const std::string& name, size_t bytes) { add_raw(n, pl, name, bytes); }
};

void plan_regnet(Plan& P) {
  // RegNet: widths are multiples of 8, the kernels read channels in slabs of 64 -- every map gets rows of
  // round_up(C, 64) channels (the input and the output of the grouped 3x3 64 more: its last group's padded slab starts
  // at channel (G - 1) * group width); the tails are zeroed with the arena below and only ever written with zeros
  const emp_pdl_config& c = P.n->cfg;
  int h = P.H / 2, w = P.W / 2;
  P.act("stem", h, w, c.rn_stem, round_up(c.rn_stem, 64));
  P.ph[0] = h; P.pw[0] = w;
  for (const RegBlock& k : P.n->reg_blocks) {
    const std::string& p = k.name;
    const int cw = k.width, ld = round_up(cw, 64);
    P.act(p + ".a", h, w, cw, ld + 64);
    const int ho = (h - 1) / k.stride + 1, wo = (w - 1) / k.stride + 1;
    P.act(p + ".b", ho, wo, cw, ld + 64);
    if (c.rn_se) {
      P.act(p + ".se1", ho, wo, round_up(cw / 4, 8), round_up(cw / 4, 64));
      P.act(p + ".se2", ho, wo, cw, ld);
    }
    if (k.shortcut) P.act(p + ".ds", ho, wo, cw, ld);
    P.act(p, ho, wo, cw, ld);
    h = ho; w = wo;
    if (k.last) { P.ph[k.si] = h; P.pw[k.si] = w; }
  }
}

void plan_resnet(Plan& P) {
  P.act("stem", P.H / 2, P.W / 2, 64);
  P.act("p1", P.H / 4, P.W / 4, 64);
  int h = P.H / 4, w = P.W / 4;
  P.ph[0] = h; P.pw[0] = w;
  for (const ResBlock& k : P.n->res_blocks) {
    const std::string& p = k.name;
    P.act(p + ".c1", h, w, k.planes);
    const int ho = (h - 1) / k.stride + 1, wo = (w - 1) / k.stride + 1;
    P.act(p + ".c2", ho, wo, k.planes);
    if (k.b == 0) P.act(p + ".ds", ho, wo, k.planes * 4);
    P.act(p, ho, wo, k.planes * 4);
    h = ho; w = wo;
    if (k.last) { P.ph[k.li] = h; P.pw[k.li] = w; }
  }
}

int plan_deeplab(Plan& P) {
  emp_pdl* n = P.n;
  const emp_pdl_config& c = n->cfg;
  const int N = P.N, h5 = P.ph[4], w5 = P.pw[4];
  P.raw("pooled", (size_t)N * 2048 * 4);
  P.raw("pool_part", (size_t)avgpool_scratch_floats(N, 2048) * 4);
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    std::string p = kDecoders[d];
    P.raw(p + ".poolfeat", (size_t)N * n->aspp_ch * 4);
    P.raw(p + ".bias_n", (size_t)N * n->aspp_ch * 4);
    P.act(p + ".aspp.cat", h5, w5, 4 * n->aspp_ch);
    P.act(p + ".aspp", h5, w5, n->aspp_ch);
    int xch = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const int st = c.low_level_stages[i];
      const int lp = d == 0 ? c.low_level_proj_sem[i] : c.low_level_proj_ins[i];
      const int cpad = round_up(xch + lp, 64);
      std::string q = p + ".stage" + std::to_string(i);
      P.act(q + ".cat", P.ph[st], P.pw[st], cpad);
      P.act(q + ".dw", P.ph[st], P.pw[st], cpad);
      P.act(q + ".out", P.ph[st], P.pw[st], n->dec_ch);
      xch = n->dec_ch;
    }
  }
  const int st_last = c.low_level_stages[c.n_stages - 1];
  P.hq = P.ph[st_last]; P.wq = P.pw[st_last];  // resolution of semantic_x (1/4 for MitoNet)
  EMP_REQUIRE(P.hq * 4 == P.H && P.wq * 4 == P.W, "the last decoder stage must be at 1/4 resolution (got %dx%d)", P.hq, P.wq);
  return EMP_OK;
}

int plan_bifpn(Plan& P) {
  emp_pdl* n = P.n;
  const emp_pdl_config& c = n->cfg;
  EMP_REQUIRE(P.H % 128 == 0 && P.W % 128 == 0, "BiFPN forward: H=%d W=%d must be multiples of 128", P.H, P.W);
  const int F = c.fpn_dim;
  P.hq = P.ph[1]; P.wq = P.pw[1];
  P.act("p2f", P.ph[1], P.pw[1], F);
  // level sizes P3..P7
  int lh[5], lw[5];
  for (int i = 0; i < 3; ++i) { lh[i] = P.ph[2 + i]; lw[i] = P.pw[2 + i]; }
  lh[3] = lh[2] / 2; lw[3] = lw[2] / 2; lh[4] = lh[3] / 2; lw[4] = lw[3] / 2;
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    std::string fp = std::string(kBifpn[d]) + "_fpn";
    P.act(fp + ".p6pre", lh[2], lw[2], F);
    P.act(fp + ".in.P6", lh[3], lw[3], F);
    P.act(fp + ".in.P7", lh[4], lw[4], F);
    for (int li = 0; li < c.fpn_layers; ++li) {
      std::string L = fp + ".l" + std::to_string(li);
      for (int lv = 0; lv < 5; ++lv) {
        std::string q = L + ".P" + std::to_string(3 + lv);
        if (li == 0 && lv < 3) { P.act(q + ".rtd", lh[lv], lw[lv], F); P.act(q + ".rbu", lh[lv], lw[lv], F); }
        const int FZ = fsplit_on(n, fp + ".") ? 2 * F : F;      // [hi | lo] pair of the fused map (emp_pdl::precise_fsplit)
        P.act(q + ".fuse", lh[lv], lw[lv], FZ);
        if (lv > 0) P.act(q + ".fuseb", lh[lv], lw[lv], FZ);   // bottom-up node's fused input (kept for taps)
        P.act(q + ".dw", lh[lv], lw[lv], F);
        P.act(q + ".td", lh[lv], lw[lv], F);
        P.act(q + ".bu", lh[lv], lw[lv], F);
      }
    }
    std::string dp = std::string(kBifpn[d]) + "_decoder";
    int hh = lh[4], ww = lw[4];
    for (int i = 0; i < 5; ++i) {
      hh *= 2; ww *= 2;
      P.act(dp + ".cat" + std::to_string(i), hh, ww, 2 * F);
    }
    P.act(dp + ".dw", P.hq, P.wq, 2 * F);
    P.act(dp + ".out", P.hq, P.wq, F);
  }
  return EMP_OK;
}

void plan_heads_pointrend(Plan& P) {
  emp_pdl* n = P.n;
  const int N = P.N;
  for (int k = 0; k < 3; ++k) {
    std::string p = kHeads[k];
    P.act(p + ".dw", P.hq, P.wq, n->dec_ch);
    P.act(p + ".pw", P.hq, P.wq, n->dec_ch);
    P.raw(p + ".out", (size_t)N * head_planes(n, k) * P.hq * P.wq * 4);
  }
  const int pts = n->cfg.subdivision_num_points;
  const int ldp = round_up(n->dec_ch + n->ncls, 64);
  int64_t plane_max = 0;
  int hh = P.hq, ww = P.wq;
  for (int s = 0; s < P.RS; ++s) {
    hh *= 2; ww *= 2;
    if (s + 1 < P.RS) P.raw("pr.sem" + std::to_string(s), (size_t)N * n->ncls * hh * ww * 4);
    plane_max = (int64_t)hh * ww;
  }
  P.raw("pr.keys", (size_t)N * plane_max * 4);
  P.raw("pr.topk", topk_work_bytes(N, plane_max));
  P.raw("pr.idx", (size_t)N * pts * 4);
  P.raw("pr.x0", (size_t)N * pts * ldp * 2);
  P.raw("pr.x1", (size_t)N * pts * ldp * 2);
}

int plan(emp_pdl* n, int N, int H, int W, int RS, hipStream_t stream) {
  const emp_pdl_config& c = n->cfg;
  EMP_REQUIRE(N > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0,
              "forward: H=%d W=%d must be positive multiples of 16 (factor_pad first)", H, W);
  EMP_REQUIRE(RS >= 1 && RS <= 6, "render_steps=%d out of range", RS);
  n->acts.clear();
  n->act_order.clear();
  n->raw.clear();
  Plan P{n, Planner(), N, H, W, RS};
  P.raw("zero", 2048);
  if (c.encoder == 1) plan_regnet(P);
  else plan_resnet(P);
  RC(c.arch == 0 ? plan_deeplab(P) : plan_bifpn(P));
  plan_heads_pointrend(P);

  const size_t need = P.pl.off;
  if (need > n->arena_cap) {
    if (n->arena) EMP_CHECK_HIP(hipFree(n->arena));
    n->arena = nullptr;
    n->arena_cap = 0;
    hipError_t e = hipMalloc((void**)&n->arena, need);
    if (e != hipSuccess) {
      set_error("arena: hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
      return EMP_ERR_NOMEM;
    }
    n->arena_cap = need;
  }
  // channel-padding regions must read as exact zeros; ordered on the caller's stream behind whatever still runs on
  // the previous layout (a hipFree above has synchronised the device already)
  EMP_CHECK_HIP(hipMemsetAsync(n->arena, 0, need, stream));
  n->arena_used = need;
  for (auto& kv : n->acts) kv.second.p = (half_t*)(n->arena + kv.second.off);
  n->pN = N; n->pH = H; n->pW = W; n->pRS = RS;
  n->capN = N;
  return EMP_OK;
}

// A smaller batch at the planned image size runs in the SAME layout: every buffer is batch-major, so the first N
// images are a prefix of it and the zero padding stays valid -- no re-plan, no re-zeroing of a multi-GB arena for
// the last partial slice chunk of a stack (and none when the full batch comes back).
void rebatch(emp_pdl* n, int N) {
  for (auto& kv : n->acts) kv.second.N = N;
  n->pN = N;
}

template <typename T>
T* rawp(emp_pdl* n, const std::string& name) {
  return (T*)(n->arena + n->raw.at(name).first);
}

// conv helper: in (channels [0,Cin_pad) of `in`), out channels [coff, coff+Cout) of `out`
struct ConvOpt {      // everything about a conv() launch beyond source, destination and stream
  int stride = 1, pad = 0, dil = 1, act = ACT_NONE;
  const Act* res = nullptr;               // residual added before the activation
  const float* bias_n = nullptr;          // per-image bias
  int ps_cout = 0;                        // pixel-shuffled output (the transposed convs): couts per sub-pixel
  const Act* in2 = nullptr;               // K-concatenated second source, sampled with stride2
  int stride2 = 1;
  const Act* out2 = nullptr;              // couts [split, Cout) go here ...
  int out2_coff = 0, split = 0;
  const Act* out3 = nullptr;              // ... and couts [split3, Cout) here
  int out3_coff = 0, split3 = 0;
  const std::string* next_name = nullptr; // back-to-back candidate: the next block's conv1, its output, "was it fused?"
  const Act* next_out = nullptr;
  bool* fused_next = nullptr;
};

int conv(emp_pdl* n, const std::string& wname, const Act& in, int in_coff, const Act& out, int out_coff, hipStream_t s,
         const ConvOpt& o = {}) {
  const auto& [stride, pad, dil, act, res, bias_n, ps_cout, in2, stride2, out2, out2_coff, split, out3, out3_coff, split3, next_name, next_out,
               fused_next] = o;      // (ConvOpt's members, in its order)
  DevConv& dc = n->convs.at(wname);
  ConvParams p{};
  if (out3) {     // couts [split3, Cout) go to a third tensor (ConvParams::out3)
    EMP_REQUIRE(out2 && out3->N == out.N && out3->H == out.H && out3->W == out.W && out3_coff + dc.cout - split3 <= out3->ld,
                "%s: third destination mismatch", wname.c_str());
    p.out3 = out3->p + out3_coff; p.out3_ld = out3->ld; p.split3 = split3;
  }
  if (out2) {     // couts [split, Cout) go to a second tensor (ConvParams::out2)
    EMP_REQUIRE(out2->N == out.N && out2->H == out.H && out2->W == out.W &&
                    out2_coff + (out3 ? split3 : dc.cout) - split <= out2->ld,
                "%s: second destination mismatch", wname.c_str());
    p.out2 = out2->p + out2_coff; p.out2_ld = out2->ld; p.split = split;
  }
  if (in2) {      // K-concatenated second source (ConvParams::in2)
    EMP_REQUIRE(dc.cin2_pad > 0 && dc.cin2_pad <= in2->ld && in2->N == in.N, "%s: second source mismatch", wname.c_str());
    p.in2 = in2->p; p.Cin2 = dc.cin2_pad; p.in2_ld = in2->ld; p.H2 = in2->H; p.W2 = in2->W; p.stride2 = stride2;
  } else {
    EMP_REQUIRE(dc.cin2_pad == 0, "%s: packed for two sources", wname.c_str());
  }
  p.in = in.p + in_coff;
  p.wgt = dc.w;
  p.bias = dc.b;
  p.bias_n = bias_n;
  p.res = res ? res->p : nullptr;
  p.res_ld = res ? res->ld : 0;
  p.out = out.p + out_coff;
  p.zero = rawp<half_t>(n, "zero");
  p.N = in.N; p.H = in.H; p.W = in.W; p.Cin = dc.cin_pad; p.in_ld = in.ld;
  p.Cout = dc.cout; p.KH = dc.kh; p.KW = dc.kw; p.stride = stride; p.pad = pad; p.dil = dil;
  p.Ho = (in.H + 2 * pad - dil * (dc.kh - 1) - 1) / stride + 1;
  p.Wo = (in.W + 2 * pad - dil * (dc.kw - 1) - 1) / stride + 1;
  const int up = ps_cout ? 2 : 1;
  EMP_REQUIRE(p.Ho * up == out.H && p.Wo * up == out.W && in.N == out.N, "%s: output shape mismatch (%dx%d vs %dx%d)",
              wname.c_str(), p.Ho * up, p.Wo * up, out.H, out.W);
  EMP_REQUIRE(in_coff + dc.cin_pad <= in.ld && out_coff + (ps_cout ? ps_cout : (out2 ? split : dc.cout)) <= out.ld,
              "%s: channel slice out of range", wname.c_str());
  p.out_ld = out.ld;
  p.act = act;
  p.ps_cout = ps_cout;
  p.M = p.N * p.Ho * p.Wo;
  double next_flops = 0.0;
  if (fused_next) *fused_next = false;
  if (next_name && n->fuse_b2b) {
    // the next bottleneck's conv1 (1x1, stride 1, ReLU) computed from this launch's tile while it is in LDS
    const DevConv& nd = n->convs.at(*next_name);
    p.next_w = nd.w; p.next_b = nd.b; p.next_out = next_out->p; p.next_cout = nd.cout; p.next_ld = next_out->ld;
    if (nd.kh == 1 && nd.kw == 1 && nd.cin_pad == dc.cout && nd.cin2_pad == 0 && next_out->N == out.N && next_out->H == out.H &&
        next_out->W == out.W && nd.cout <= next_out->ld && out_coff == 0 && conv_b2b_supported(p)) {
      *fused_next = true;
      next_flops = 2.0 * (double)p.M * nd.cout * (double)nd.cin;
      n->flops += next_flops;
    } else {
      p.next_w = nullptr; p.next_b = nullptr; p.next_out = nullptr; p.next_cout = 0; p.next_ld = 0;
    }
  }
  const double kflop = (double)(dc.cin * dc.kh * dc.kw + (dc.wsplit ? 0 : dc.cin2));      // a hi + lo weight pair is one product
  n->flops += 2.0 * (double)p.M * dc.cout * kflop;
  if (n->layer_log)   // EMP_LAYER_LOG=<file>: one line per MFMA launch, in launch order (tools/layer_roofline.py)
    fprintf(n->layer_log, "conv,%s,%d,%d,%d,%d,%d,%d,%d,%d\n", wname.c_str(), p.M, dc.cin_pad + dc.cin2_pad, dc.cout, dc.kh,
            stride, dil, res ? 1 : 0, in.N * in.H * in.W);
  int variant = 0;
  if (n->pack256 && !p.next_w && conv_uses_256(p)) {
    // the 256 x 256 tile reads its weights from a packed image (whole 128-byte lines per LDS-DMA instruction): made once,
    // at the first launch of this layer that takes the tile (batch-dependent), on the launch's stream
    // (round 6, ADVICE r05: the images are made by emp_pdl_finalize for every layer whose SHAPE the tile takes -- no allocation,
    // no device synchronisation and no failure mode inside a forward; a layer without one runs the tile on its plain weights)
    if (dc.w256) {
      p.wgt = dc.w256;
      variant = 1 << 20;
    }
  }
  if (n->profile && !p.next_w && conv_uses_256(p)) {     // the fused back-to-back launches are another kernel symbol
    return profiled_launch(n, s, 2.0 * (double)p.M * dc.cout * kflop, [&] { return launch_conv_igemm(p, variant, s); });
  }
  return launch_conv_igemm(p, variant, s);
}

// One separable block of the fp16 engine -- depthwise ks x ks -> pointwise -> act [-> the head's 1x1] -- with the parameters
// base + "0" / base + "1" (pwc: the packed base + "1"): the kernel with the exact depthwise half (sepconv_precise.hip) where the site asks for it, else the
// fused kernel (sepconv.hip: neither the depthwise nor, at a head, the pointwise map reaches HBM), else the depthwise launch
// into acts[tmp + ".dw"] and conv() (at a head through acts[tmp + ".pw"] and launch_head1x1).  The caller has booked the
// depthwise flops; the fused paths book the pointwise flops here, the fallback's come from conv().
struct SepBlock {
  int ks = 5, act = ACT_RELU;
  bool precise = false;          // precise_node / precise_layer of this block
  bool hilo = false;             // BiFPN node whose fused map arrives as channels [hi | lo]: always the precise kernel
  int64_t min_tiles = 0;         // the fused (NOT the precise) kernel only from this many 8 x 16 tiles (BiFPN nodes)
  const Act* out = nullptr;      // the block's output map; a head has none and, instead, its 1x1:
  const float* head_w = nullptr;
  const float* head_b = nullptr;
  int hc = 0;
  float* head_dst = nullptr;
};

int sepblock(emp_pdl* n, const std::string& base, const DevConv& pwc, const std::string& logname, const Act& in, int C,
             const std::string& tmp, const half_t* zero, hipStream_t s, const SepBlock& b) {
  const bool head = !b.out;
  const int N = in.N, M = N * in.H * in.W, out_ld = head ? 0 : b.out->ld;
  half_t* outp = head ? nullptr : b.out->p;
  const int64_t plane = head ? (int64_t)in.H * in.W : 0;
  const bool fits = head ? in.C == C && pwc.cin_pad == C && pwc.cout == C && b.hc <= 2 : pwc.cin_pad == C && in.ld == C && out_ld == pwc.cout;
  auto book = [&](const char* tag) {      // (tools/layer_roofline.py parses the line)
    n->flops += 2.0 * (double)N * in.H * in.W * pwc.cout * (double)pwc.cin;
    if (n->layer_log) fprintf(n->layer_log, "%s,%s,%d,%d,%d,%d,1,1,0,%d\n", tag, logname.c_str(), M, C, pwc.cout, b.ks, M);
  };
  if (b.hilo || (n->fuse_sepconv && b.precise)) {
    auto pk = n->f16w.find(base + (b.hilo ? "1.packedpd" : "1.packedp"));
    if (pk != n->f16w.end() && (b.hilo || (fits && sepconvp_supported(C, pwc.cout, b.hc)))) {
      RC(launch_sepconvp(in.p, N, in.H, in.W, C, in.ld, n->f32w.at(base + (b.hilo ? "0.f32d" : "0.f32")), pk->second, pwc.b, pwc.cout, b.act,
                         outp, out_ld, b.head_w, b.head_b, b.hc, b.head_dst, plane, zero, s, b.ks, pwc.wsplit ? 1 : 0));
      book(head ? "sepheadp" : "sepconvp");
      return EMP_OK;
    }
  }
  if (n->fuse_sepconv && fits && (int64_t)N * ((in.H + 7) / 8) * ((in.W + 15) / 16) >= b.min_tiles) {
    auto pk = n->f16w.find(base + "1.packed");
    if (pk != n->f16w.end() && sepconv5_supported(C, pwc.cout, b.hc)) {
      RC(launch_sepconv5(in.p, N, in.H, in.W, C, in.ld, n->f16w.at(base + "0"), pk->second, pwc.b, pwc.cout, b.act, outp, out_ld, b.head_w,
                         b.head_b, b.hc, b.head_dst, plane, zero, s, b.ks));
      book(head ? "sephead" : "sepconv");
      return EMP_OK;
    }
  }
  const Act& dw = n->acts.at(tmp + ".dw");
  RC(launch_dwconv(in.p, N, in.H, in.W, C, in.ld, n->f16w.at(base + "0"), b.ks, dw.p, dw.ld, zero, s));
  if (!head) return conv(n, base + "1", dw, 0, *b.out, 0, s, {.act = b.act});
  const Act& pw = n->acts.at(tmp + ".pw");
  RC(conv(n, base + "1", dw, 0, pw, 0, s, {.act = b.act}));
  return launch_head1x1(pw.p, N, in.H * in.W, C, C, b.head_w, b.head_b, b.hc, b.head_dst, plane, nullptr, s);
}

// One forward of the fp16 engine: what its stages share
struct Fwd : Forward {
  bool par;               // the instance side runs on the second stream (emp_pdl::aux); s: the caller's stream
  const half_t* zero;
  std::string xname;
  bool proj_done[8] = {false, false, false, false, false, false, false, false};   // decoder projections written by the encoder

  Act& A(const std::string& k) { return n->acts.at(k); }
  hipStream_t side(bool ins) const { return (par && ins) ? n->aux : s; }
  int fork() {      // everything both decoders read is enqueued on s: the second stream starts here
    if (!par) return EMP_OK;
    EMP_CHECK_HIP(hipEventRecord(n->ev_fork, s));
    EMP_CHECK_HIP(hipStreamWaitEvent(n->aux, n->ev_fork, 0));
    return EMP_OK;
  }
  int regnet_grouped3x3(const RegBlock& k);
  int regnet_encoder();
  int resnet_encoder();
  int bifpn_decoders();
  int aspp_and_projections(const Act& p5, bool aspp_done[4]);
  int deeplab_decoders();
  int heads();
  int pointrend();
};

// one launch, blockIdx.y = group (conv_igemm_grouped.hip): Cout = the group width exactly, Cin = it padded to 64
int Fwd::regnet_grouped3x3(const RegBlock& k) {
  const std::string& p = k.name;
  const int cw = k.width, g = k.groups, gw = cw / g, sb = k.stride;
  const DevConv& dc = n->convs.at(p + ".bottleneck.b.0#grouped");
  const Act& in = A(p + ".a");
  const Act& out = A(p + ".b");
  ConvParams q{};
  q.in = in.p; q.wgt = dc.w; q.bias = dc.b; q.out = out.p; q.zero = rawp<half_t>(n, "zero");
  q.N = in.N; q.H = in.H; q.W = in.W; q.Cin = dc.cin_pad; q.in_ld = in.ld;
  q.Cout = gw; q.KH = 3; q.KW = 3; q.stride = sb; q.pad = 1; q.dil = 1;
  q.Ho = (in.H + 2 - 3) / sb + 1;
  q.Wo = (in.W + 2 - 3) / sb + 1;
  EMP_REQUIRE(q.Ho == out.H && q.Wo == out.W && in.N == out.N, "%s: grouped 3x3 output shape mismatch", p.c_str());
  q.out_ld = out.ld; q.act = 1; q.M = q.N * q.Ho * q.Wo;
  n->flops += 2.0 * (double)q.M * cw * (double)(gw * 9);
  return launch_conv_igemm_grouped(q, g, gw, (long long)gw * 9 * dc.cin_pad, gw, s);
}

// RegNet (regnet.py:160-166) on the generic conv: a (1x1) -> b (grouped 3x3) -> [per-pixel squeeze-excite gate] -> c (1x1) +
// shortcut, ReLU
int Fwd::regnet_encoder() {
  const Act& st = A("stem");
  RC(launch_stem3x3s2_f16(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("rn.stem.w"), n->f32w.at("rn.stem.b"), c.rn_stem, st.p,
                          st.ld, s));
  n->flops += 2.0 * N * (H / 2) * (W / 2) * (double)c.rn_stem * 9.0;
  xname = "stem";
  pyr[0] = "stem";
  for (const RegBlock& k : n->reg_blocks) {
    const std::string& p = k.name;
    const int cw = k.width, g = k.groups, gw = cw / g, sb = k.stride;
    RC(conv(n, p + ".bottleneck.a.0", A(xname), 0, A(p + ".a"), 0, s, {.act = ACT_RELU}));
    // one grouped launch, unless every group alone already fills the chip with the register-weight 3x3 kernel's tiles
    // (stride 1, >= 2048 tiles of 8 x 16 pixels: the big maps of a big batch, where that kernel is the faster one)
    const Act& ain = A(p + ".a");
    const bool per_group = !n->regnet_grouped || (sb == 1 && (int64_t)N * cdiv(ain.H, 8) * cdiv(ain.W, 16) >= n->regnet_group_tiles);
    if (!per_group) {
      RC(regnet_grouped3x3(k));
    } else {
      for (int gi = 0; gi < g; ++gi)
        RC(conv(n, p + ".bottleneck.b.0#" + std::to_string(gi), A(p + ".a"), gi * gw, A(p + ".b"), gi * gw, s,
            {.stride = sb, .pad = 1, .act = ACT_RELU}));
    }
    if (c.rn_se) {
      RC(conv(n, p + ".bottleneck.se.se.0#pad", A(p + ".b"), 0, A(p + ".se1"), 0, s, {.act = ACT_RELU}));
      RC(conv(n, p + ".bottleneck.se.se.2", A(p + ".se1"), 0, A(p + ".se2"), 0, s));
      const Act& xb = A(p + ".b");      // the gated map lands in .se2 (the gate's own buffer); .b keeps the pre-gate map
      RC(launch_gate_mul_f16(xb.p, xb.ld, A(p + ".se2").p, A(p + ".se2").ld, (int64_t)N * xb.H * xb.W, cw, s));
    }
    const Act* idn = &A(xname);
    if (k.shortcut) {
      RC(conv(n, p + ".downsample.conv.0", A(xname), 0, A(p + ".ds"), 0, s, {.stride = sb}));
      idn = &A(p + ".ds");
    }
    RC(conv(n, p + ".bottleneck.c.0", A(p + (c.rn_se ? ".se2" : ".b")), 0, A(p), 0, s, {.act = ACT_RELU, .res = idn}));
    xname = p;
    if (k.last) pyr[k.si] = p;
  }
  return EMP_OK;
}

int Fwd::resnet_encoder() {
  if (n->fuse_stem) {
    // conv1 + bn1 + relu + maxpool in one launch on the matrix pipe; the half-resolution map is never written
    RC(launch_stem_pool(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("stem.w"), n->f32w.at("stem.b"), A("p1").p, s));
  } else {
    RC(launch_stem7x7(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("stem.w"), n->f32w.at("stem.b"), A("stem").p, s));
    RC(launch_maxpool3x3s2(A("stem").p, N, H / 2, W / 2, 64, A("p1").p, s));
  }
  n->flops += 2.0 * N * (H / 2) * (W / 2) * 64.0 * 49.0;
  xname = "p1";
  pyr[0] = "p1";
  bool c1_done = false;      // the coming block's conv1 was computed by the previous block's last launch
  for (const ResBlock& k : n->res_blocks) {
    const std::string& p = k.name;
    if (!c1_done) {
      // first block of a stage whose input the decoders project too: one conv, three destinations (see finalize)
      int pi = -1;
      if (k.b == 0 && c.arch == 0)
        for (int i = 0; i < c.n_stages; ++i)
          if (c.low_level_stages[i] == k.li - 1 && n->convs.count(p + ".conv1+project." + std::to_string(i))) pi = i;
      if (pi >= 0) {
        const int xch = pi == 0 ? n->aspp_ch : n->dec_ch;      // where the projected channels sit in the concat buffers
        const Act& cb1 = A(std::string(kDecoders[0]) + ".stage" + std::to_string(pi) + ".cat");
        const Act& cb2 = A(std::string(kDecoders[1]) + ".stage" + std::to_string(pi) + ".cat");
        const int c1 = n->convs.at(p + ".conv1").cout;
        RC(conv(n, p + ".conv1+project." + std::to_string(pi), A(xname), 0, A(p + ".c1"), 0, s,
            {.act = ACT_RELU, .out2 = &cb1, .out2_coff = xch, .split = c1, .out3 = &cb2, .out3_coff = xch, .split3 = c1 + c.low_level_proj_sem[pi]}));
        proj_done[pi] = true;
      } else {
        RC(conv(n, p + ".conv1", A(xname), 0, A(p + ".c1"), 0, s, {.act = ACT_RELU}));
      }
    }
    c1_done = false;
    RC(conv(n, p + ".conv2", A(p + ".c1"), 0, A(p + ".c2"), 0, s, {.stride = k.stride, .pad = k.dil, .dil = k.dil, .act = ACT_RELU}));
    // the conv1 of the block that follows (same layer, or the first block of the next one): a candidate for the
    // back-to-back fusion into this block's last launch (ConvParams::next_*; conv() decides)
    const std::string nxt_w = k.next + ".conv1";
    const bool has_next = !k.next.empty() && n->convs.count(nxt_w);
    const std::string* next_name = has_next ? &nxt_w : nullptr;
    const Act* next_out = has_next ? &A(k.next + ".c1") : nullptr;
    if (k.b == 0 && n->fuse_ds) {
      // relu(bn3(conv3(c2)) + bn(downsample(x))) as ONE GEMM whose K runs over c2's channels and then over x's
      // (sampled with the block's stride): the shortcut map is neither written nor read back
      RC(conv(n, p + ".conv3+ds", A(p + ".c2"), 0, A(p), 0, s,
          {.act = ACT_RELU, .in2 = &A(xname), .stride2 = k.stride, .next_name = next_name, .next_out = next_out, .fused_next = &c1_done}));
    } else {
      const Act* idn = &A(xname);
      if (k.b == 0) {
        RC(conv(n, p + ".downsample.0", A(xname), 0, A(p + ".ds"), 0, s, {.stride = k.stride}));
        idn = &A(p + ".ds");
      }
      RC(conv(n, p + ".conv3", A(p + ".c2"), 0, A(p), 0, s,
          {.act = ACT_RELU, .res = idn, .next_name = next_name, .next_out = next_out, .fused_next = &c1_done}));
    }
    xname = p;
    if (k.last) pyr[k.li] = p;
  }
  return EMP_OK;
}

// ---- BiFPN decoders (bifpn.py:185-236, panoptic_bifpn.py:70-82) ----
int Fwd::bifpn_decoders() {
  const int F = c.fpn_dim;
  RC(conv(n, "p2_resample.conv.0", A(pyr[1]), 0, A("p2f"), 0, s));
  RC(fork());
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    hipStream_t s = side(d == 1);
    const std::string fp = std::string(kBifpn[d]) + "_fpn";
    // P6 / P7 (bifpn.py:187-188)
    RC(conv(n, fp + ".p6_resample.conv.0", A(pyr[4]), 0, A(fp + ".p6pre"), 0, s));
    {
      const Act& a6 = A(fp + ".p6pre");
      RC(launch_maxpool3x3s2(a6.p, N, a6.H, a6.W, F, A(fp + ".in.P6").p, s));
      const Act& b6 = A(fp + ".in.P6");
      RC(launch_maxpool3x3s2(b6.p, N, b6.H, b6.W, F, A(fp + ".in.P7").p, s));
    }
    std::string feat[5] = {pyr[2], pyr[3], pyr[4], fp + ".in.P6", fp + ".in.P7"};   // P3..P7
    auto resample = [&](const std::string& rk, const std::string& src, const std::string& dst, std::string* name) -> int {
      *name = src;
      if (!n->convs.count(rk)) return EMP_OK;
      *name = dst;
      return conv(n, rk, A(src), 0, A(dst), 0, s);
    };
    auto node = [&](const std::string& dirpre, const std::string& q, const std::string& a, const std::string& b2, const std::string& c3,
                    float ca, float cb, float cc, int mode, const std::string& outname) -> int {
      const half_t *pa = A(a).p, *pb = A(b2).p, *pc = c3.empty() ? nullptr : A(c3).p;
      const Act& fz = A(q + (mode ? ".fuseb" : ".fuse"));
      const std::string base = dirpre + ".after_combines.0.0.sepconv.", pwn = base + "1";
      const DevConv& pwc = n->convs.at(pwn);
      const Act& on = A(outname);
      n->flops += 2.0 * 9.0 * (double)N * fz.H * fz.W * F;
      // fused map as an fp16 hi + lo pair in channels [0, F) | [F, 2F); the node's block reads all 2F with duplicated
      // taps and pointwise weights (fsplit_on): always fused, one rounding sequence at every batch size
      const bool hilo = fz.ld == 2 * F && n->f16w.count(pwn + ".packedpd") && on.ld == pwc.cout;
      if (hilo) RC(launch_fuse_combine(pa, pb, pc, ca, cb, cc, mode, N, fz.H, fz.W, F, fz.p, s, fz.p + F, 2 * F));
      else RC(launch_fuse_combine(pa, pb, pc, ca, cb, cc, mode, N, fz.H, fz.W, F, fz.p, s));
      // the 3x3 block with the exact depthwise half (precise_node) runs fused at EVERY size -- the kernel is the only
      // implementation of its rounding sequence, so no tile-count threshold may pick another one; the plain fused kernel
      // (sepconv.hip, KS = 3) once the map has a tile per CU
      return sepblock(n, base, pwc, pwn, fz, hilo ? 2 * F : F, q, zero, s,
                      {.ks = 3, .act = ACT_SILU, .precise = precise_node(n, pwn), .hilo = hilo, .min_tiles = n->sepconv_min_tiles, .out = &on});
    };
    for (int li = 0; li < c.fpn_layers; ++li)
      RC(bifpn_layer(n, fp + ".bifpns." + std::to_string(li), fp + ".l" + std::to_string(li), feat, resample, node));
    // decoder: 5 x (ConvTranspose k2 s2 + BN + ReLU, concat skip), 5x5 separable fusion (bifpn.py:226-236)
    const std::string dp = std::string(kBifpn[d]) + "_decoder";
    const std::string skips[5] = {feat[3], feat[2], feat[1], feat[0], "p2f"};
    std::string x = feat[4];
    for (int i = 0; i < 5; ++i) {
      const Act& cat = A(dp + ".cat" + std::to_string(i));
      const std::string un = dp + ".upsamplings." + std::to_string(i) + ".0";
      RC(conv(n, un, A(x), 0, cat, 0, s, {.act = ACT_RELU, .ps_cout = F, .in2 = n->convs.at(un).wsplit ? &A(x) : nullptr}));
      const Act& sk = A(skips[i]);
      RC(launch_bilinear_ac(sk.p, N, sk.H, sk.W, F, sk.ld, cat.p + F, cat.H, cat.W, cat.ld, s));  // same size: strided copy
      x = dp + ".cat" + std::to_string(i);
    }
    const Act& cat = A(x);
    n->flops += 2.0 * 25.0 * (double)N * cat.H * cat.W * 2 * F;
    // the decoder that feeds the centre heat-map (precise_layer): the block with the exact depthwise half
    const std::string fu = dp + ".fusion.0";
    RC(sepblock(n, fu + ".sepconv.", n->convs.at(fu + ".sepconv.1"), fu, cat, 2 * F, dp, zero, s,
                {.precise = precise_layer(n, fu), .out = &A(dp + ".out")}));
    dec_out[d] = dp + ".out";
  }
  return EMP_OK;
}

// what both Panoptic-DeepLab decoders read and the launches that serve both, all on s in front of the fork
int Fwd::aspp_and_projections(const Act& p5, bool aspp_done[4]) {
  RC(launch_avgpool(p5.p, N, p5.H * p5.W, p5.C, p5.ld, rawp<float>(n, "pooled"), rawp<float>(n, "pool_part"), s));
  // ASPP branches of BOTH decoders, one conv per branch (couts [0, aspp_ch) -> semantic concat buffer, the rest ->
  // instance concat buffer) when the merged weights exist (finalize) and the launch goes to the 256x256 tile
  const bool aspp_merged = c.ins_decoder && (int64_t)((N * p5.H * p5.W + 255) / 256) * (2 * n->aspp_ch / 256) >= 192;
  if (aspp_merged)      // smaller problems keep the separate launches (deep-ring 64x64 tile, two streams)
    for (int i = 0; i <= 3; ++i) {
      const std::string pm = "decoders.aspp.convs." + std::to_string(i) + ".0";
      if (!n->convs.count(pm)) continue;
      const int r = i == 0 ? 1 : c.atrous_rates[i - 1];
      const Act& cat0 = A(std::string(kDecoders[0]) + ".aspp.cat");
      const Act& cat1 = A(std::string(kDecoders[1]) + ".aspp.cat");
      RC(conv(n, pm, p5, 0, cat0, i * n->aspp_ch, s,
          {.pad = i == 0 ? 0 : r, .dil = r, .act = ACT_RELU, .out2 = &cat1, .out2_coff = i * n->aspp_ch, .split = n->aspp_ch}));
      aspp_done[i] = true;
    }
  // The merged low-level projections ("decoders.project.i": one pass over a pyramid level writes BOTH decoders' concat
  // buffers) that the encoder did not already run: they read encoder maps only and must be on s BEFORE the
  // instance side forks onto the second stream -- after the fork nothing would order the instance decoder's read of
  // its concat buffer behind this launch (EMP_FUSE_PROJ=0, low_level_stages with stage 0, odd conv1 shapes).
  if (c.ins_decoder) {
    int xch0 = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const std::string pm = "decoders.project." + std::to_string(i);
      if (!proj_done[i] && n->convs.count(pm)) {
        const Act& cb1 = A(std::string(kDecoders[0]) + ".stage" + std::to_string(i) + ".cat");
        const Act& cb2 = A(std::string(kDecoders[1]) + ".stage" + std::to_string(i) + ".cat");
        RC(conv(n, pm, A(pyr[c.low_level_stages[i]]), 0, cb1, xch0, s,
            {.act = ACT_RELU, .out2 = &cb2, .out2_coff = xch0, .split = c.low_level_proj_sem[i]}));
        proj_done[i] = true;
      }
      xch0 = n->dec_ch;
    }
  }
  return EMP_OK;
}

// ---- Panoptic-DeepLab decoders ----
int Fwd::deeplab_decoders() {
  const Act& p5 = A(pyr[4]);
  bool aspp_done[4] = {false, false, false, false};
  RC(aspp_and_projections(p5, aspp_done));
  RC(fork());
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    hipStream_t s = side(d == 1);
    std::string p = kDecoders[d];
    float* poolfeat = rawp<float>(n, p + ".poolfeat");
    float* bias_n = rawp<float>(n, p + ".bias_n");
    RC(launch_gemv(rawp<float>(n, "pooled"), N, p5.C, n->f32w.at(p + ".pool.w"), nullptr, n->aspp_ch, 1, poolfeat, s));
    RC(launch_gemv(poolfeat, N, n->aspp_ch, n->f32w.at(p + ".projpool.w"), nullptr, n->aspp_ch, 0, bias_n, s));
    const Act& cat = A(p + ".aspp.cat");
    if (!aspp_done[0]) RC(conv(n, p + ".aspp.convs.0.0", p5, 0, cat, 0, s, {.act = ACT_RELU}));
    for (int i = 1; i <= 3; ++i) {
      if (aspp_done[i]) continue;
      const int r = c.atrous_rates[i - 1];
      RC(conv(n, p + ".aspp.convs." + std::to_string(i) + ".0", p5, 0, cat, i * n->aspp_ch, s, {.pad = r, .dil = r, .act = ACT_RELU}));
    }
    RC(conv(n, p + ".aspp.project.0", cat, 0, A(p + ".aspp"), 0, s, {.act = ACT_RELU, .bias_n = bias_n}));
    std::string x = p + ".aspp";
    int xch = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const int st = c.low_level_stages[i];
      std::string q = p + ".stage" + std::to_string(i);
      const Act& cb = A(q + ".cat");
      const Act& xa = A(x);
      RC(launch_bilinear_ac(xa.p, N, xa.H, xa.W, xch, xa.ld, cb.p, cb.H, cb.W, cb.ld, s));
      // (proj_done: written by the encoder's merged launch -- conv1 of the next stage + both projections -- or by the merged
      // projection in front of the fork)
      if (!proj_done[i]) RC(conv(n, p + ".project." + std::to_string(i) + ".0", A(pyr[st]), 0, cb, xch, s, {.act = ACT_RELU}));
      const std::string fz = p + ".fuse." + std::to_string(i) + ".0.sepconv.";
      n->flops += 2.0 * 25.0 * (double)N * cb.H * cb.W * (xch + n->convs.at(p + ".project." + std::to_string(i) + ".0").cout);
      // the decoder that feeds the centre heat-map (precise_layer): the block with the exact depthwise half
      RC(sepblock(n, fz, n->convs.at(fz + "1"), fz, cb, cb.ld, q, zero, s, {.precise = precise_layer(n, p + ".fuse." + std::to_string(i) + ".0"), .out = &A(q + ".out")}));
      x = q + ".out";
      xch = n->dec_ch;
    }
    dec_out[d] = x;
  }
  return EMP_OK;
}

// ---- heads: head.0 (depthwise 5x5 -> pointwise -> ReLU) and head.1 (1x1 -> head_planes); the instance heads on the second stream ----
int Fwd::heads() {
  const Act& semx = A(dec_out[0]);
  const Act& insx = A(dec_out[1]);
  const int hq = semx.H, wq = semx.W;
  for (int k = 0; k < 3; ++k) {
    hipStream_t s = side(k > 0);
    std::string p = kHeads[k];
    const int hc = head_planes(n, k);
    const Act& xin = k == 0 ? semx : insx;
    n->flops += 2.0 * 25.0 * (double)N * hq * wq * n->dec_ch;
    float* dst = rawp<float>(n, p + ".out");
    if (k == 1 && !interp) dst = o_ctr;
    if (k == 2 && !interp) dst = o_off;
    head_out[k] = dst;
    // the centre head (precise_layer) with the exact depthwise half
    RC(sepblock(n, p + ".head.0.0.sepconv.", n->convs.at(p + ".head.0.0.sepconv.1"), p, xin, n->dec_ch, p, zero, s,
                {.precise = precise_layer(n, p + ".head.0.0"), .head_w = n->f32w.at(p + ".head.1.w"), .head_b = n->f32w.at(p + ".head.1.b"),
                 .hc = hc, .head_dst = dst}));
    n->flops += 2.0 * (double)N * hq * wq * n->dec_ch * hc;
  }
  if (interp) {
    hipStream_t s = side(true);
    RC(launch_bilinear_ac_f32_nchw(head_out[1], N * 1, hq, wq, o_ctr, 4, s));
    RC(launch_bilinear_ac_f32_nchw(head_out[2], N * 2, hq, wq, o_off, 4, s));
  }
  if (par) EMP_CHECK_HIP(hipEventRecord(n->ev_join, n->aux));      // joined at the end: PointRend overlaps the instance heads
  return EMP_OK;
}

// ---- PointRend subdivision ----
int Fwd::pointrend() {
  const Act& semx = A(dec_out[0]);
  const int hq = semx.H, wq = semx.W;
  const int P = c.subdivision_num_points;
  const int ldp = round_up(n->dec_ch + n->ncls, 64);
  const float* coarse = head_out[0];
  const float* cur = coarse;
  int hh = hq, ww = wq;
  uint32_t* keys = rawp<uint32_t>(n, "pr.keys");
  int32_t* idx = rawp<int32_t>(n, "pr.idx");
  half_t* X[2] = {rawp<half_t>(n, "pr.x0"), rawp<half_t>(n, "pr.x1")};
  for (int st = 0; st < RS; ++st) {
    float* nxt = (st + 1 < RS) ? rawp<float>(n, "pr.sem" + std::to_string(st)) : o_sem;
    RC(launch_upsample2x_keys(cur, N, n->ncls, hh, ww, nxt, keys, s));
    hh *= 2; ww *= 2;
    const int64_t plane = (int64_t)hh * ww;
    const int k = (int)(plane < P ? plane : P);
    RC(launch_topk_smallest(keys, N, plane, k, rawp<char>(n, "pr.topk"), n->raw.at("pr.topk").second, idx, s));
    if (n->fuse_pr && pr_mlp_supported(n->dec_ch, ldp, n->ncls, c.num_fc)) {
      // sampling + fc layers + predictor + scatter in one launch: the (points x ldp) rows stay in LDS
      const half_t* fw_[4];
      const float* fb_[4];
      for (int f = 0; f < c.num_fc; ++f) {
        const DevConv& dc = n->convs.at("semantic_pr.point_head.fc_layers." + std::to_string(f) + ".0");
        fw_[f] = dc.w; fb_[f] = dc.b;
        n->flops += 2.0 * (double)N * k * dc.cout * (double)dc.cin;
      }
      RC(launch_pr_mlp(semx.p, N, hq, wq, n->dec_ch, semx.ld, coarse, n->ncls, idx, k, hh, ww, fw_, fb_, c.num_fc, ldp,
                       n->f32w.at("pr.predictor.w"), n->f32w.at("pr.predictor.b"), nxt, plane, s));
      n->flops += 2.0 * (double)N * k * ldp * n->ncls;
      cur = nxt;
      continue;
    }
    RC(launch_point_features(semx.p, N, hq, wq, n->dec_ch, semx.ld, coarse, n->ncls, idx, k, hh, ww, X[0], X[1], ldp, s));
    Act xa[2];
    for (int j = 0; j < 2; ++j) {
      xa[j].p = X[j]; xa[j].N = 1; xa[j].H = 1; xa[j].W = N * k; xa[j].C = ldp; xa[j].ld = ldp;
    }
    int curx = 0;
    for (int f = 0; f < c.num_fc; ++f) {
      RC(conv(n, "semantic_pr.point_head.fc_layers." + std::to_string(f) + ".0", xa[curx], 0, xa[curx ^ 1], 0, s, {.act = ACT_RELU}));
      curx ^= 1;
    }
    RC(launch_head1x1(X[curx], N, k, ldp, ldp, n->f32w.at("pr.predictor.w"), n->f32w.at("pr.predictor.b"), n->ncls, nxt,
                      plane, idx, s));
    n->flops += 2.0 * (double)N * k * ldp * n->ncls;
    cur = nxt;
  }
  return EMP_OK;
}

int run(emp_pdl* n, const void* img, int dtype, float sub, float mul, int N, int H, int W, int vh, int vw, int RS,
        int interp, float* o_sem, float* o_ctr, float* o_off, hipStream_t s) {
  const emp_pdl_config& c = n->cfg;
  n->flops = 0.0;
  const bool par = c.ins_decoder && (int64_t)N * H * W <= n->par_limit;
  if (par && !n->aux) {
    EMP_CHECK_HIP(hipStreamCreateWithFlags(&n->aux, hipStreamNonBlocking));
    EMP_CHECK_HIP(hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming));
    EMP_CHECK_HIP(hipEventCreateWithFlags(&n->ev_join, hipEventDisableTiming));
  }
  Fwd f{{n, c, img, dtype, sub, mul, N, H, W, vh, vw, RS, interp, o_sem, o_ctr, o_off, s}, par, rawp<half_t>(n, "zero")};
  RC(c.encoder == 1 ? f.regnet_encoder() : f.resnet_encoder());
  RC(c.arch == 1 ? f.bifpn_decoders() : f.deeplab_decoders());
  if (!c.ins_decoder) f.dec_out[1] = f.dec_out[0];
  RC(f.heads());
  RC(f.pointrend());
  // the caller's stream owns every output again once the instance side has finished
  if (par) EMP_CHECK_HIP(hipStreamWaitEvent(s, n->ev_join, 0));
  return EMP_OK;
}

// ---- the bodies of the C entries below; the entries run them under guarded() ----

int create(const emp_pdl_config* cfg, emp_pdl_t** out) {
  EMP_REQUIRE(cfg && out, "pdl_create: null argument");
  EMP_REQUIRE(cfg->num_classes >= 1 && cfg->num_classes <= 8, "num_classes=%d unsupported", cfg->num_classes);
  EMP_REQUIRE(cfg->stage4_stride == 16 || cfg->stage4_stride == 32, "stage4_stride must be 16 or 32");
  EMP_REQUIRE(cfg->arch == 0 || cfg->arch == 1, "arch must be 0 (PanopticDeepLabPR) or 1 (PanopticBiFPNPR)");
  if (cfg->arch == 1) {
    EMP_REQUIRE(cfg->fpn_dim > 0 && cfg->fpn_dim % 64 == 0 && cfg->fpn_layers >= 1 && cfg->stage4_stride == 32,
                "BiFPN: fpn_dim must be a multiple of 64, fpn_layers >= 1, stage4_stride 32");
  } else {
    EMP_REQUIRE(cfg->n_stages >= 1 && cfg->n_stages <= 3, "n_stages=%d unsupported", cfg->n_stages);
    EMP_REQUIRE(cfg->decoder_channels % 64 == 0 && cfg->decoder_channels > 0, "decoder_channels must be a multiple of 64");
  }
  EMP_REQUIRE(cfg->num_fc >= 1 && cfg->subdivision_num_points > 0, "bad PointRend configuration");
  for (int i = 0; i < (cfg->arch == 0 ? cfg->n_stages : 0); ++i) {
    EMP_REQUIRE(cfg->low_level_stages[i] >= 1 && cfg->low_level_stages[i] <= 3, "low_level_stages[%d] out of range", i);
    EMP_REQUIRE(cfg->low_level_proj_sem[i] % 8 == 0 && (!cfg->ins_decoder || cfg->low_level_proj_ins[i] % 8 == 0),
                "projected low-level channels must be multiples of 8");
  }
  EMP_REQUIRE(cfg->encoder == 0 || cfg->encoder == 1, "encoder must be 0 (ResNet50) or 1 (RegNet)");
  if (cfg->encoder == 1) {
    EMP_REQUIRE(cfg->rn_stem > 0 && cfg->rn_stem % 4 == 0, "RegNet: stem width %d must be a positive multiple of 4", cfg->rn_stem);
    for (int i = 0; i < 4; ++i) {
      const int w = cfg->rn_widths[i], g = cfg->rn_groups[i];
      EMP_REQUIRE(w > 0 && g > 0 && w % g == 0 && (w / g) % 4 == 0 && w % 8 == 0 && cfg->rn_depths[i] >= 1 &&
                      (cfg->rn_strides[i] == 1 || cfg->rn_strides[i] == 2),
                  "RegNet stage %d: width %d (multiple of 8), groups %d (group width a multiple of 4), depth %d, stride %d", i + 1, w, g,
                  cfg->rn_depths[i], cfg->rn_strides[i]);
    }
    int os_ = 2;
    for (int i = 0; i < 4; ++i) os_ *= cfg->rn_strides[i];
    EMP_REQUIRE(cfg->rn_strides[0] == 2 && (os_ == 32 || os_ == 16) && (cfg->arch == 0 || os_ == 32),
                "RegNet: stage 1 must be at stride 4 and the encoder's output stride 16 or 32 (BiFPN: 32)");
  }
  std::unique_ptr<emp_pdl> n(new emp_pdl());
  n->cfg = *cfg;
  n->dec_ch = cfg->arch == 1 ? cfg->fpn_dim : cfg->decoder_channels;
  n->aspp_ch = cfg->aspp_channels > 0 ? cfg->aspp_channels : cfg->decoder_channels;
  n->ncls = cfg->num_classes;
  if (cfg->encoder == 1) n->reg_blocks = regnet_blocks(*cfg);
  else n->res_blocks = resnet_blocks(*cfg);
  build_param_list(n.get());
  *out = n.release();
  return EMP_OK;
}

int set_param(emp_pdl_t* net, const char* name, const float* h_w, const int64_t* shape, int ndim,
                      const float* h_b) {
  EMP_REQUIRE(net && name && h_w && shape, "set_param: null argument");
  auto it = net->params.find(name);
  EMP_REQUIRE(it != net->params.end(), "set_param: unknown parameter '%s'", name);
  EMP_REQUIRE(ndim == 1 || ndim == 3 || ndim == 4, "set_param(%s): ndim must be 1, 3 or 4", name);
  HostParam& hp = it->second;
  hp.shape.assign(shape, shape + ndim);
  size_t cnt = 1;
  for (int i = 0; i < ndim; ++i) {
    EMP_REQUIRE(shape[i] > 0, "set_param(%s): non-positive dimension", name);
    cnt *= (size_t)shape[i];
  }
  hp.w.assign(h_w, h_w + cnt);
  hp.b.assign((size_t)shape[0], 0.f);
  if (h_b) hp.b.assign(h_b, h_b + shape[0]);
  hp.set = true;
  net->finalized = false;
  return EMP_OK;
}

int tap(emp_pdl_t* net, const char* name, void** d_ptr, int64_t shape5[5]) {
  EMP_REQUIRE(net && name && d_ptr && shape5, "tap: null argument");
  auto it = net->acts.find(name);
  EMP_REQUIRE(it != net->acts.end(), "tap: unknown activation '%s'", name);
  const Act& a = it->second;
  *d_ptr = a.p;
  shape5[0] = a.N; shape5[1] = a.H; shape5[2] = a.W; shape5[3] = a.C; shape5[4] = a.ld;
  return EMP_OK;
}

int tap_raw(emp_pdl_t* net, const char* name, void** d_ptr, int64_t* bytes) {
  EMP_REQUIRE(net && name && d_ptr && bytes, "tap_raw: null argument");
  if (net->fp32_graph()) {      // fp32 / fp16x3 mode: every buffer of the last forward by name (maps: NHWC fp32)
    auto it32 = net->pool32.find(name);
    EMP_REQUIRE(it32 != net->pool32.end(), "tap_raw: unknown fp32 buffer '%s'", name);
    *d_ptr = it32->second.first;
    *bytes = (int64_t)(it32->second.second * sizeof(float));
    return EMP_OK;
  }
  auto it = net->raw.find(name);
  EMP_REQUIRE(it != net->raw.end(), "tap_raw: unknown buffer '%s'", name);
  *d_ptr = net->arena + it->second.first;
  *bytes = (int64_t)it->second.second;
  return EMP_OK;
}

// ---- emp_pdl_finalize's stages (fp16 engine; the fp32 graph's weights: finalize32) ----

// a parameter that exists for one pack only (merged, padded or sliced weights), under the name its launch looks up
int pack_as(emp_pdl* n, const std::string& name, const HostParam& hp) { return pack_conv(n, name, 0, &hp); }

// [a ; b] along Cout (same input channels and kernel size): the weights of one launch with two destinations
HostParam concat_cout(const HostParam& a, const HostParam& b) {
  HostParam m;
  m.shape = a.shape;
  m.shape[0] = a.shape[0] + b.shape[0];
  m.w = a.w;
  m.w.insert(m.w.end(), b.w.begin(), b.w.end());
  m.b = a.b;
  m.b.insert(m.b.end(), b.b.begin(), b.b.end());
  return m;
}

// couts [first, first + rows) of a conv parameter, zero-padded to rows_to couts (zero weights, zero bias)
HostParam padded_cout(const HostParam& hp, size_t first, size_t rows, size_t rows_to) {
  const size_t per = hp.w.size() / (size_t)hp.shape[0];
  HostParam t;
  t.shape = hp.shape;
  t.shape[0] = (int64_t)rows_to;
  t.w.assign(rows_to * per, 0.f);
  std::copy(hp.w.begin() + first * per, hp.w.begin() + (first + rows) * per, t.w.begin());
  t.b.assign(rows_to, 0.f);
  std::copy(hp.b.begin() + first, hp.b.begin() + first + rows, t.b.begin());
  return t;
}

// The pooled ASPP branch of decoder p as the matrices of two GEMVs: the pooling conv (aspp, 2048) and the projection's (aspp, 5*aspp)
// last aspp input channels, which enter as a per-image bias; head: its first 4*aspp input channels, a conv of the concat buffer
int upload_aspp_pool(emp_pdl* n, const std::string& p, HostParam* head) {
  const int A = n->aspp_ch;
  RC(upload_f32(n, p + ".pool.w", n->params[p + ".aspp.convs.4.aspp_pooling.1"].w));
  const HostParam& hp = n->params[p + ".aspp.project.0"];
  EMP_REQUIRE(hp.shape[0] == A && hp.shape[1] == 5 * A, "%s.aspp.project.0 must be (%d,%d,1,1)", p.c_str(), A, 5 * A);
  std::vector<float> tail;
  split_aspp_project(hp, A, head, &tail);
  return upload_f32(n, p + ".projpool.w", tail);
}

// RegNet in the fp32 / fp16x3 mode: none of the fp16 packs; what run32 reads besides finalize32's conv weights
int finalize_regnet_fp32(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  if (c.arch == 1) {
    for (const auto& nm : n->param_names)
      if (nm.size() > 8 && nm.compare(nm.size() - 8, 8, ".weights") == 0) RC(set_fusew(n, nm));
  } else {
    for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
      HostParam head;
      RC(upload_aspp_pool(n, kDecoders[d], &head));
    }
  }
  RC(upload_heads_f32(n));
  return finalize32(n);
}

// RegNet on the fp16 engine (regnet.py:38-160): every layer on the generic implicit-GEMM conv (conv_igemm.hip); the
// grouped 3x3 as one launch per group on a channel slice (group width 56 / 72 -> K padded to 64 / 128 with zero
// weights, Cout = the group width); the squeeze convolution's width (w / 4) padded to a multiple of 8 with zero rows
int finalize_regnet(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  RC(upload_regnet_stem(n));
  for (const RegBlock& k : n->reg_blocks) {
    const std::string& p = k.name;
    const int w = k.width, g = k.groups, gw = w / g;
    RC(pack_conv(n, p + ".bottleneck.a.0"));
    const HostParam& hb = n->params.at(p + ".bottleneck.b.0");
    EMP_REQUIRE(hb.shape.size() == 4 && hb.shape[0] == w && hb.shape[1] == gw && hb.shape[2] == 3 && hb.shape[3] == 3 && gw % 8 == 0,
                "%s.bottleneck.b.0 must be (%d,%d,3,3) with a group width that is a multiple of 8", p.c_str(), w, gw);
    // a group's couts padded to its K padding (56 -> 64, 72 -> 128) with zero rows and zero bias: a 64 -> 64 / 128 -> 128
    // 3x3 is what the register-weight kernels take (conv3x3c64.hip, ~1 PFLOP/s on ResNet layer1's conv2).  The zeros
    // a group writes past its width land on the first channels of the NEXT group -- whose launch follows on the
    // same stream and overwrites them -- or, for the last group, on the row's zero tail
    for (int gi = 0; gi < g; ++gi)
      RC(pack_as(n, p + ".bottleneck.b.0#" + std::to_string(gi), padded_cout(hb, (size_t)gi * gw, gw, round_up(gw, 64))));
    // ... and all groups in one blob [g][gw][9][gw padded to 64] for the grouped launch (no cout padding: a group
    // stores its own couts only, the groups run side by side)
    RC(pack_as(n, p + ".bottleneck.b.0#grouped", hb));
    if (c.rn_se) {
      // zero rows + zero bias for the padded squeeze channels: relu(0) = 0 meets zero input weights
      const HostParam& h0 = n->params.at(p + ".bottleneck.se.se.0");
      HostParam t = padded_cout(h0, 0, (size_t)h0.shape[0], round_up((int)h0.shape[0], 8));
      t.shape = {t.shape[0], h0.shape[1], 1, 1};
      RC(pack_as(n, p + ".bottleneck.se.se.0#pad", t));
      RC(pack_conv(n, p + ".bottleneck.se.se.2"));
    }
    RC(pack_conv(n, p + ".bottleneck.c.0"));
    if (k.shortcut) RC(pack_conv(n, p + ".downsample.conv.0"));
  }
  return EMP_OK;
}

int finalize_resnet(emp_pdl* n) {
  // stem: (64,1,7,7) -> [49][64] fp32
  const HostParam& hp = n->params["encoder.conv1"];
  EMP_REQUIRE(hp.shape.size() == 4 && hp.shape[0] == 64 && hp.shape[1] == 1 && hp.shape[2] == 7 && hp.shape[3] == 7,
              "encoder.conv1 must be (64,1,7,7)");
  std::vector<float> w(49 * 64);
  for (int o = 0; o < 64; ++o)
    for (int t = 0; t < 49; ++t) w[t * 64 + o] = hp.w[o * 49 + t];
  RC(upload_f32(n, "stem.w", w));
  RC(upload_f32(n, "stem.b", hp.b));
  for (const ResBlock& k : n->res_blocks) {
    const std::string& p = k.name;
    RC(pack_conv(n, p + ".conv1"));
    RC(pack_conv(n, p + ".conv2"));
    RC(pack_conv(n, p + ".conv3"));
    if (k.b == 0) {
      RC(pack_conv(n, p + ".downsample.0"));
      RC(pack_conv3_ds(n, p));
    }
  }
  return EMP_OK;
}

int finalize_bifpn(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  const int F = c.fpn_dim;
  RC(pack_conv(n, "p2_resample.conv.0"));
  for (const auto& nm : n->param_names) {
    const bool fpn = nm.find("_fpn.") != std::string::npos, dec = nm.find("_decoder.") != std::string::npos;
    if (!fpn && !dec) continue;
    if (nm.size() > 8 && nm.compare(nm.size() - 8, 8, ".weights") == 0) {
      RC(set_fusew(n, nm));
    } else if (nm.find(".sepconv.0") != std::string::npos) {
      const HostParam& hp = n->params[nm];
      RC(pack_dw(n, nm, round_up((int)hp.shape[0], 64), nm.find(".after_combines.") != std::string::npos && fsplit_on(n, nm)));
    } else if (nm.find(".upsamplings.") != std::string::npos) {
      const char* cdec = c.ins_decoder ? "instance_decoder." : "semantic_decoder.";
      RC(pack_convT(n, nm, wsplit_on(n) && nm.compare(0, strlen(cdec), cdec) == 0));
      EMP_REQUIRE(n->convs[nm].cout == 4 * F, "%s: transposed conv must produce fpn_dim channels", nm.c_str());
    } else {
      RC(pack_conv(n, nm));
      if (nm.size() > 19 && nm.compare(nm.size() - 19, 19, ".fusion.0.sepconv.1") == 0) {
        RC(pack_sepconv_pw(n, nm));
        if (precise_layer(n, nm.substr(0, nm.size() - 10))) RC(pack_sepconvp_pw(n, nm));
      }
      if (nm.find(".after_combines.0.0.sepconv.1") != std::string::npos) {      // BiFPN nodes
        RC(pack_sepconv_pw(n, nm));
        if (fsplit_on(n, nm)) RC(pack_sepconvp_pw(n, nm, true));
        else if (precise_node(n, nm)) RC(pack_sepconvp_pw(n, nm));
      }
    }
  }
  return EMP_OK;
}

// the two decoders' low-level projections of one pyramid level as ONE conv with two destinations
int finalize_merged_projections(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  for (int i = 0; i < c.n_stages; ++i) {
    const HostParam& hs = n->params.at(std::string(kDecoders[0]) + ".project." + std::to_string(i) + ".0");
    const HostParam& hi = n->params.at(std::string(kDecoders[1]) + ".project." + std::to_string(i) + ".0");
    if (hs.shape[1] != hi.shape[1] || hs.shape[0] % 8 != 0) continue;
    HostParam m = concat_cout(hs, hi);
    m.shape = {m.shape[0], hs.shape[1], 1, 1};
    RC(pack_as(n, "decoders.project." + std::to_string(i), m));
    // ... and, when that level is a ResNet stage output whose next consumer is the following stage's first conv1 (a
    // 1x1 conv of the same map), all THREE as one conv with three destinations: the map (the widest the projections
    // read: 1 GiB per 32 tiles at stride 4) is read once instead of twice
    const int st = c.low_level_stages[i];
    const std::string c1n = "encoder.layer" + std::to_string(st + 1) + ".0.conv1";
    if (n->fuse_proj && st >= 1 && st < 4 && n->params.count(c1n)) {
      const HostParam& h1 = n->params.at(c1n);
      if (h1.shape.size() == 4 && h1.shape[2] == 1 && h1.shape[3] == 1 && h1.shape[1] == hs.shape[1] && h1.shape[0] % 8 == 0)
        RC(pack_as(n, c1n + "+project." + std::to_string(i), concat_cout(h1, m)));
    }
  }
  return EMP_OK;
}

int finalize_deeplab(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    std::string p = kDecoders[d];
    for (int i = 0; i <= 3; ++i) RC(pack_conv(n, p + ".aspp.convs." + std::to_string(i) + ".0"));
    if (d == 1 && n->fuse_aspp) {
      // both decoders' ASPP branch i read the same stride-16 map: one conv of 2 x aspp_ch couts, the second 256-cout
      // tile lands in the instance decoder's concat buffer (ConvParams::out2); the pixel tile is fetched once
      for (int i = 0; i <= 3; ++i) {
        const std::string b = ".aspp.convs." + std::to_string(i) + ".0";
        const HostParam& hs = n->params.at(std::string(kDecoders[0]) + b);
        const HostParam& hi = n->params.at(std::string(kDecoders[1]) + b);
        if (hs.shape != hi.shape || hs.shape[0] % 256 != 0) continue;
        RC(pack_as(n, "decoders" + b, concat_cout(hs, hi)));
      }
    }
    HostParam head;
    RC(upload_aspp_pool(n, p, &head));
    RC(pack_as(n, p + ".aspp.project.0", head));
    int xch = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const int lp = d == 0 ? c.low_level_proj_sem[i] : c.low_level_proj_ins[i];
      const int cpad = round_up(xch + lp, 64);
      const std::string fz = p + ".fuse." + std::to_string(i) + ".0";
      RC(pack_conv(n, p + ".project." + std::to_string(i) + ".0"));
      EMP_REQUIRE(n->convs[p + ".project." + std::to_string(i) + ".0"].cout == lp, "%s.project.%d: Cout != %d", p.c_str(), i, lp);
      RC(pack_dw(n, fz + ".sepconv.0", cpad));
      RC(pack_conv(n, fz + ".sepconv.1", cpad));
      RC(pack_sepconv_pw(n, fz + ".sepconv.1"));
      if (precise_layer(n, fz)) RC(pack_sepconvp_pw(n, fz + ".sepconv.1"));
      xch = n->dec_ch;
    }
  }
  if (n->fuse_ds && c.ins_decoder) RC(finalize_merged_projections(n));
  return EMP_OK;
}

int finalize_heads_pointrend(emp_pdl* n) {
  for (int k = 0; k < 3; ++k) {
    std::string p = kHeads[k];
    RC(pack_dw(n, p + ".head.0.0.sepconv.0", n->dec_ch));
    RC(pack_conv(n, p + ".head.0.0.sepconv.1"));
    RC(pack_sepconv_pw(n, p + ".head.0.0.sepconv.1"));
    if (precise_layer(n, p + ".head.0.0")) RC(pack_sepconvp_pw(n, p + ".head.0.0.sepconv.1"));
  }
  RC(upload_heads_f32(n));
  const int ldp = round_up(n->dec_ch + n->ncls, 64);
  for (int k = 0; k < n->cfg.num_fc; ++k) RC(pack_conv(n, "semantic_pr.point_head.fc_layers." + std::to_string(k) + ".0", ldp));
  return upload_f32(n, "pr.predictor.w", padded_predictor(n->params["semantic_pr.point_head.predictor"], n->ncls, ldp));
}

// packed weight images of the 256 x 256 tile (whole 128-byte lines per LDS-DMA instruction; conv_igemm256.hip pack256_kernel) for
// every layer whose shape the tile takes at SOME batch: Cout % 256 == 0, 64-channel granularity along K, K >= 512 (conv_uses_256's
// floor; K >= 128 with a second source).  A second copy of the layer3 / layer4 / ASPP weights (~90 MB; emp_pdl_arena_bytes
// counts activations only, as before).
int finalize_images256(emp_pdl* n) {
  for (auto& kv : n->convs) {
    DevConv& dc = kv.second;
    const int K = dc.kh * dc.kw * dc.cin_pad + dc.cin2_pad;
    if (dc.w256 || !dc.w || dc.cout % 256 != 0 || dc.cin_pad % 64 != 0 || dc.cin2_pad % 64 != 0 || K < (dc.cin2_pad ? 128 : 512)) continue;
    const size_t halfs = (size_t)dc.cout * K;
    RC(dev_alloc(n, halfs, &dc.w256));
    n->image_bytes += halfs * sizeof(half_t);
    const int prc = conv256_pack_weights(dc.w, dc.w256, dc.cout, dc.kh * dc.kw, dc.cin_pad, dc.cin2_pad, nullptr);
    if (prc) return prc;
  }
  EMP_CHECK_HIP(hipStreamSynchronize(nullptr));
  return EMP_OK;
}

int finalize(emp_pdl* n) {
  for (const auto& nm : n->param_names)
    if (!n->params[nm].set) {
      set_error("finalize: parameter '%s' was never set", nm.c_str());
      return EMP_ERR_STATE;
    }
  const emp_pdl_config& c = n->cfg;
  if (c.encoder == 1 && n->fp32_graph()) {
    RC(finalize_regnet_fp32(n));
    n->finalized = true;
    return EMP_OK;
  }
  RC(c.encoder == 1 ? finalize_regnet(n) : finalize_resnet(n));
  RC(c.arch == 1 ? finalize_bifpn(n) : finalize_deeplab(n));
  RC(finalize_heads_pointrend(n));
  if (n->fp32_graph()) RC(finalize32(n));      // fp32 reference mode: fp32 copies of every weight
  if (n->pack256 && !n->fp32_graph()) RC(finalize_images256(n));
  n->finalized = true;
  return EMP_OK;
}

}  // namespace

extern "C" {

int emp_pdl_create(const emp_pdl_config* cfg, emp_pdl_t** out) {
  return guarded("emp_pdl_create", [&] { return create(cfg, out); });
}

void emp_pdl_destroy(emp_pdl_t* net) { delete net; }

int emp_pdl_num_params(const emp_pdl_t* net) { return net ? (int)net->param_names.size() : 0; }
const char* emp_pdl_param_name(const emp_pdl_t* net, int i) {
  if (!net || i < 0 || i >= (int)net->param_names.size()) return nullptr;
  return net->param_names[i].c_str();
}

int emp_pdl_set_param(emp_pdl_t* net, const char* name, const float* h_w, const int64_t* shape, int ndim,
                      const float* h_b) {
  return guarded("emp_pdl_set_param", [&] { return set_param(net, name, h_w, shape, ndim, h_b); });
}

int emp_pdl_finalize(emp_pdl_t* n) {
  EMP_REQUIRE(n, "finalize: null network");
  return guarded("emp_pdl_finalize", [&] { return finalize(n); });
}

int emp_pdl_set_precision(emp_pdl_t* net, int precision) {
  EMP_REQUIRE(net, "set_precision: null network");
  EMP_REQUIRE(precision >= 0 && precision <= 2, "set_precision: 0 = fp16 engine, 1 = fp32 reference mode, 2 = fp16x3 mode (got %d)", precision);
  EMP_REQUIRE(!net->finalized, "set_precision: call before emp_pdl_finalize");
  net->precision = precision;
  return EMP_OK;
}
int emp_pdl_precision(const emp_pdl_t* net) { return net ? net->precision : -1; }

int emp_pdl_reserve(emp_pdl_t* net, int N, int H, int W) {
  EMP_REQUIRE(net, "reserve: null network");
  if (net->fp32_graph()) return EMP_OK;      // the fp32 / fp16x3 modes size its buffers on first use
  return guarded("emp_pdl_reserve", [&] { return plan(net, N, H, W, net->pRS > 2 ? net->pRS : 2, nullptr); });
}
size_t emp_pdl_arena_bytes(const emp_pdl_t* net) { return net ? net->arena_used : 0; }

int emp_pdl_forward_padded(emp_pdl_t* net, const void* d_image, int image_dtype, float sub, float mul, int N, int vh, int vw,
                           int H, int W, int render_steps, int interpolate_ins, float* d_sem_logits, float* d_ctr_hmp,
                           float* d_offsets, void* stream) {
  EMP_REQUIRE(net && d_image && d_sem_logits && d_ctr_hmp && d_offsets, "forward: null argument");
  EMP_REQUIRE(vh > 0 && vw > 0 && vh <= H && vw <= W, "forward: valid size %dx%d must fit the padded size %dx%d", vh, vw, H, W);
  if (!net->finalized) {
    set_error("forward: call emp_pdl_finalize first");
    return EMP_ERR_STATE;
  }
  return guarded("emp_pdl_forward", [&]() -> int {
    hipStream_t s = (hipStream_t)stream;
    if (net->fp32_graph())
      return run32(net, d_image, image_dtype, sub, mul, N, H, W, vh, vw, render_steps, interpolate_ins, d_sem_logits, d_ctr_hmp, d_offsets, s);
    if (H != net->pH || W != net->pW || render_steps != net->pRS || N > net->capN) {
      RC(plan(net, N, H, W, render_steps, s));
    } else if (N != net->pN) {
      rebatch(net, N);
    }
    const int rc = run(net, d_image, image_dtype, sub, mul, N, H, W, vh, vw, render_steps, interpolate_ins, d_sem_logits, d_ctr_hmp, d_offsets, s);
    if (net->layer_log) { fprintf(net->layer_log, "end\n"); fflush(net->layer_log); }
    return rc;
  });
}

int emp_pdl_forward(emp_pdl_t* net, const void* d_image, int image_dtype, float sub, float mul, int N, int H, int W,
                    int render_steps, int interpolate_ins, float* d_sem_logits, float* d_ctr_hmp, float* d_offsets,
                    void* stream) {
  return emp_pdl_forward_padded(net, d_image, image_dtype, sub, mul, N, H, W, H, W, render_steps, interpolate_ins,
                                d_sem_logits, d_ctr_hmp, d_offsets, stream);
}

double emp_pdl_flops(const emp_pdl_t* net, int, int, int, int) { return net ? net->flops : 0.0; }

int emp_pdl_profile(emp_pdl_t* net, int enable) {
  EMP_REQUIRE(net != nullptr, "profile: null network");
  net->profile = enable != 0;
  net->prof_used = 0;
  net->prof_flops = 0.0;
  return EMP_OK;
}

int emp_pdl_profile_read(emp_pdl_t* net, double* ms_total, double* flops_total, int* launches) {
  EMP_REQUIRE(net && ms_total && flops_total && launches, "profile_read: null pointer");
  double ms = 0.0;
  for (size_t i = 0; i < net->prof_used; ++i) {
    float t = 0.f;
    EMP_CHECK_HIP(hipEventSynchronize(net->prof_events[i].second));
    EMP_CHECK_HIP(hipEventElapsedTime(&t, net->prof_events[i].first, net->prof_events[i].second));
    ms += t;
  }
  *ms_total = ms;
  *flops_total = net->prof_flops;
  *launches = (int)net->prof_used;
  net->prof_used = 0;
  net->prof_flops = 0.0;
  return EMP_OK;
}

int emp_pdl_num_taps(const emp_pdl_t* net) { return net ? (int)net->act_order.size() : 0; }
const char* emp_pdl_tap_name(const emp_pdl_t* net, int i) {
  if (!net || i < 0 || i >= (int)net->act_order.size()) return nullptr;
  return net->act_order[i].c_str();
}
int emp_pdl_tap(emp_pdl_t* net, const char* name, void** d_ptr, int64_t shape5[5]) {
  return guarded("emp_pdl_tap", [&] { return tap(net, name, d_ptr, shape5); });
}

int emp_pdl_tap_raw(emp_pdl_t* net, const char* name, void** d_ptr, int64_t* bytes) {
  return guarded("emp_pdl_tap_raw", [&] { return tap_raw(net, name, d_ptr, bytes); });
}

int emp_pdl_num_maps32(const emp_pdl_t* net) { return net ? (int)net->maps32.size() : 0; }
int emp_pdl_map32(const emp_pdl_t* net, int i, const char** name, const char** kind, void** d_ptr, int64_t shape5[5], int* fmt) {
  EMP_REQUIRE(net && name && kind && d_ptr && shape5 && fmt, "map32: null argument");
  EMP_REQUIRE(i >= 0 && i < (int)net->maps32.size(), "map32: index %d out of range (%d buffers in the last forward)", i, (int)net->maps32.size());
  const emp_pdl::Map32& m = net->maps32[i];
  *name = m.name.c_str(); *kind = m.kind.c_str(); *d_ptr = m.p; *fmt = m.fmt;
  shape5[0] = m.N; shape5[1] = m.H; shape5[2] = m.W; shape5[3] = m.C; shape5[4] = m.ld;
  return EMP_OK;
}

}  // extern "C"
