// The fp32 reference mode and the fp16x3 mode of the network scheduler (pdl_net.h; the fp16 schedule and the C entries:
// pdl_net.hip): fp32 weight packers, finalize32, the conv helper c32 and the layer schedule run32.
#include "pdl_net.h"

namespace {

// ======================================================================================================================
// fp32 reference mode (round 4).  The same layer schedule as run() -- panoptic_deeplab.py:194-250 / panoptic_bifpn.py:147-161
// in eval -- with every map and weight in fp32 and no layer fusion: one generic exact-fp32 MFMA conv (ref32.hip), the
// depthwise / pooling / resampling layers on the fp32 vector pipe.  The ASPP pooling branch still enters the projection
// as a per-image bias (exact algebra, aspp.py:45-48,99-102).  Slow by design: the device-side fp32 comparator.
// ======================================================================================================================
struct T32 { float* p = nullptr; int N = 0, H = 0, W = 0, C = 0, ld = 0; int fmt = 0; };      // fmt 1: an hl32 map (conv16x3p.hip), same bytes

int buf32(emp_pdl* n, const std::string& key, size_t floats, float** out) {
  auto it = n->pool32.find(key);
  if (it == n->pool32.end() || it->second.second < floats) {
    if (it != n->pool32.end()) { EMP_CHECK_HIP(hipFree(it->second.first)); n->pool32.erase(it); }
    float* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, floats * sizeof(float) + 64);
    if (e != hipSuccess) {
      set_error("fp32 mode: hipMalloc(%zu bytes) for '%s' failed: %s", floats * sizeof(float), key.c_str(), hipGetErrorString(e));
      return EMP_ERR_NOMEM;
    }
    EMP_CHECK_HIP(hipMemset(d, 0, floats * sizeof(float)));      // channel pads must read as zeros
    n->pool32[key] = {d, floats};
    *out = d;
    return EMP_OK;
  }
  *out = it->second.first;
  return EMP_OK;
}

// the forward's record of a buffer it made (emp_pdl::maps32): a name made twice in one forward keeps its place, with the later geometry
void note32(emp_pdl* n, const std::string& name, const char* kind, float* p, int64_t N, int64_t H, int64_t W, int64_t C, int64_t ld, int fmt = 0) {
  auto at = n->maps32_at.find(name);
  if (at == n->maps32_at.end()) {
    n->maps32_at.emplace(name, n->maps32.size());
    n->maps32.push_back({name, kind, p, N, H, W, C, ld, fmt});
    return;
  }
  emp_pdl::Map32& m = n->maps32[at->second];
  m.kind = kind; m.p = p; m.N = N; m.H = H; m.W = W; m.C = C; m.ld = ld; m.fmt = fmt;
}

int t32(emp_pdl* n, const std::string& key, int N, int H, int W, int C, T32* t) {
  t->N = N; t->H = H; t->W = W; t->C = C; t->ld = C;
  return buf32(n, key, (size_t)N * H * W * C, &t->p);
}

// packed weights and bias to the device, the conv under its name
int store32(emp_pdl* n, const std::string& name, emp_pdl::W32 w, const std::vector<float>& pk, const std::vector<float>& b) {
  RC(dev_upload(n, pk.data(), pk.size() * sizeof(float), (void**)&w.w));
  RC(dev_upload(n, b.data(), b.size() * sizeof(float), (void**)&w.b));
  n->w32[name] = w;
  return EMP_OK;
}

// OIHW / OIW fp32 -> [O][KH*KW][I16] fp32 (+ bias); cin_to: pad the input channels to this many (PointRend rows)
int pack32(emp_pdl* n, const std::string& name, int cin_to = 0, const HostParam* src = nullptr) {
  const HostParam& hp = src ? *src : n->params.at(name);
  EMP_REQUIRE(hp.shape.size() == 4 || hp.shape.size() == 3, "%s: conv weight must be 3-d or 4-d", name.c_str());
  emp_pdl::W32 w;
  w.cout = (int)hp.shape[0];
  w.cin = (int)hp.shape[1];
  w.kh = hp.shape.size() == 4 ? (int)hp.shape[2] : 1;
  w.kw = hp.shape.size() == 4 ? (int)hp.shape[3] : 1;
  w.cin16 = cin_to ? cin_to : round_up(w.cin, 16);
  EMP_REQUIRE(w.cin16 >= w.cin && w.cin16 % 16 == 0, "%s: bad channel padding", name.c_str());
  const int kt = w.kh * w.kw;
  std::vector<float> pk((size_t)w.cout * kt * w.cin16, 0.f);
  for (int o = 0; o < w.cout; ++o)
    for (int i = 0; i < w.cin; ++i)
      for (int t = 0; t < kt; ++t) pk[((size_t)o * kt + t) * w.cin16 + i] = hp.w[((size_t)o * w.cin + i) * kt + t];
  return store32(n, name, w, pk, hp.b);
}

// fp16x3 mode: conv3 and the projection shortcut of a bottleneck as one fp32 weight matrix [Cout][cin3_16 | cin_ds_16] with
// the summed (folded BN) bias -- relu(conv3(c2) + downsample(x)) as a single convolution over the concatenated K
// (Conv32::in2; the fp16 engine's pack_conv3_ds): the shortcut map is neither written nor read back
int pack32_conv3_ds(emp_pdl* n, const std::string& block) {
  emp_pdl::W32 w;
  std::vector<float> pk, b;
  RC(concat_conv3_ds(n, block, 16, &w.cout, &w.cin, &w.cin16, &w.cin2, &w.cin2_16, &pk, &b));
  return store32(n, block + ".conv3+ds", w, pk, b);
}

// depthwise (C,1,k,k) -> [k*k][C] fp32
int pack32_dw(emp_pdl* n, const std::string& name, int cpad) {
  const HostParam& hp = n->params.at(name);
  const int C = (int)hp.shape[0], KK = (int)(hp.shape[2] * hp.shape[3]);
  EMP_REQUIRE(cpad >= C, "%s: bad depthwise padding", name.c_str());
  std::vector<float> pk((size_t)KK * cpad, 0.f);
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < KK; ++t) pk[(size_t)t * cpad + c] = hp.w[(size_t)c * KK + t];
  return upload_f32(n, name + ".dw32", pk);
}

// ConvTranspose2d(k=2,s=2) weight (Cin,Cout,2,2) -> 1x1 conv with 4*Cout outputs, fp32 (pack_convT)
int pack32_convT(emp_pdl* n, const std::string& name) {
  const HostParam& hp = n->params.at(name);
  EMP_REQUIRE(hp.shape.size() == 4 && hp.shape[2] == 2 && hp.shape[3] == 2, "%s: expected (Cin,Cout,2,2)", name.c_str());
  const int cin = (int)hp.shape[0], co = (int)hp.shape[1];
  HostParam t;
  t.shape = {4 * co, cin, 1, 1};
  t.w.resize((size_t)4 * co * cin);
  t.b.resize((size_t)4 * co);
  for (int q = 0; q < 4; ++q)
    for (int o = 0; o < co; ++o) {
      t.b[(size_t)q * co + o] = hp.b[o];
      for (int i = 0; i < cin; ++i) t.w[((size_t)q * co + o) * cin + i] = hp.w[(((size_t)i * co + o) * 2 + (q >> 1)) * 2 + (q & 1)];
    }
  return pack32(n, name, 0, &t);
}

// [wa ; wb] stacked along Cout (same kernel size and padded Cin): the fp32 weights and biases of ONE launch with two destinations
int stack32(emp_pdl* n, const emp_pdl::W32& wa, const emp_pdl::W32& wb, emp_pdl::W32* m) {
  *m = wa;
  m->cout = wa.cout + wb.cout; m->wp = nullptr; m->wimg = nullptr; m->wimgp = nullptr;
  const size_t K = (size_t)wa.kh * wa.kw * wa.cin16, na = (size_t)wa.cout * K, nb = (size_t)wb.cout * K;
  RC(dev_alloc(n, na + nb, &m->w));
  EMP_CHECK_HIP(hipMemcpy(m->w, wa.w, na * sizeof(float), hipMemcpyDeviceToDevice));
  EMP_CHECK_HIP(hipMemcpy(m->w + na, wb.w, nb * sizeof(float), hipMemcpyDeviceToDevice));
  RC(dev_alloc(n, (size_t)m->cout, &m->b));
  EMP_CHECK_HIP(hipMemcpy(m->b, wa.b, (size_t)wa.cout * sizeof(float), hipMemcpyDeviceToDevice));
  EMP_CHECK_HIP(hipMemcpy(m->b + wa.cout, wb.b, (size_t)wb.cout * sizeof(float), hipMemcpyDeviceToDevice));
  return EMP_OK;
}

// ---- finalize32's stages ----

int pack32_encoder(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  if (c.encoder == 1) RC(upload_regnet_stem(n));
  for (const RegBlock& k : n->reg_blocks) {
    const std::string& p = k.name;
    const int w = k.width, g = k.groups;
    RC(pack32(n, p + ".bottleneck.a.0"));
    RC(pack32(n, p + ".bottleneck.b.0"));      // (w, w / g, 3, 3): rows [o][tap][(w / g) padded to 16], group-major in o
    const emp_pdl::W32& wb = n->w32.at(p + ".bottleneck.b.0");
    EMP_REQUIRE(wb.cout == w && wb.cin * g == w && wb.kh == 3 && wb.kw == 3, "%s.bottleneck.b.0 must be (%d,%d,3,3)", p.c_str(), w,
                w / g);
    if (c.rn_se) {
      RC(pack32(n, p + ".bottleneck.se.se.0"));
      RC(pack32(n, p + ".bottleneck.se.se.2"));
    }
    RC(pack32(n, p + ".bottleneck.c.0"));
    if (k.shortcut) RC(pack32(n, p + ".downsample.conv.0"));
  }
  for (const ResBlock& k : n->res_blocks) {
    const std::string& p = k.name;
    RC(pack32(n, p + ".conv1"));
    RC(pack32(n, p + ".conv2"));
    RC(pack32(n, p + ".conv3"));
    if (k.b == 0) RC(pack32(n, p + ".downsample.0"));
    if (k.b == 0 && n->precision == 2) RC(pack32_conv3_ds(n, p));
  }
  return EMP_OK;
}

int pack32_bifpn(emp_pdl* n) {
  RC(pack32(n, "p2_resample.conv.0"));
  for (const auto& nm : n->param_names) {
    const bool fpn = nm.find("_fpn.") != std::string::npos, dec = nm.find("_decoder.") != std::string::npos;
    if (!fpn && !dec) continue;
    if (nm.size() > 8 && nm.compare(nm.size() - 8, 8, ".weights") == 0) continue;      // fusew: host side (finalize)
    if (nm.find(".sepconv.0") != std::string::npos) RC(pack32_dw(n, nm, (int)n->params[nm].shape[0]));
    else if (nm.find(".upsamplings.") != std::string::npos) RC(pack32_convT(n, nm));
    else RC(pack32(n, nm));
  }
  return EMP_OK;
}

int pack32_deeplab(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    const std::string p = kDecoders[d];
    for (int i = 0; i <= 3; ++i) RC(pack32(n, p + ".aspp.convs." + std::to_string(i) + ".0"));
    // projection: first 4A input channels -> conv; the pooled branch's A channels -> per-image bias (projpool.w)
    HostParam head;
    std::vector<float> tail;
    split_aspp_project(n->params[p + ".aspp.project.0"], n->aspp_ch, &head, &tail);
    RC(pack32(n, p + ".aspp.project.0", 0, &head));
    int xch = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const int lp = d == 0 ? c.low_level_proj_sem[i] : c.low_level_proj_ins[i];
      RC(pack32(n, p + ".project." + std::to_string(i) + ".0"));
      const int cpad = round_up(xch + lp, n->precision == 2 ? 32 : 16);      // (the fused block walks the channels in chunks of 32)
      RC(pack32_dw(n, p + ".fuse." + std::to_string(i) + ".0.sepconv.0", cpad));
      RC(pack32(n, p + ".fuse." + std::to_string(i) + ".0.sepconv.1", cpad));
      xch = n->dec_ch;
    }
  }
  return EMP_OK;
}

int pack32_heads_pointrend(emp_pdl* n) {
  for (int k = 0; k < 3; ++k) {
    const std::string p = kHeads[k];
    RC(pack32_dw(n, p + ".head.0.0.sepconv.0", n->dec_ch));
    RC(pack32(n, p + ".head.0.0.sepconv.1"));
  }
  const int ldp = round_up(n->dec_ch + n->ncls, 16);
  for (int k = 0; k < n->cfg.num_fc; ++k) RC(pack32(n, "semantic_pr.point_head.fc_layers." + std::to_string(k) + ".0", ldp));
  return upload_f32(n, "pr.predictor.w32", padded_predictor(n->params["semantic_pr.point_head.predictor"], n->ncls, ldp));
}

// fp16x3 mode, round 6: the separable blocks' weights in the fused kernel's orders (sepconv_x3.hip)
int x3_sep_weights(emp_pdl* n) {
  for (auto& kv : n->w32) {
    const std::string& nm = kv.first;
    if (nm.size() < 10 || nm.compare(nm.size() - 10, 10, ".sepconv.1") != 0) continue;
    const std::string base = nm.substr(0, nm.size() - 2);      // "... .sepconv"
    auto dwi = n->f32w.find(base + ".0.dw32");
    auto hpi = n->params.find(base + ".0");
    if (dwi == n->f32w.end() || hpi == n->params.end() || hpi->second.shape.size() != 4) continue;
    const emp_pdl::W32& w = kv.second;
    const int ks = (int)hpi->second.shape[2], C = w.cin16;
    if (w.kh != 1 || w.kw != 1 || !sepconv_x3_supported(C, w.cout, 0, ks)) continue;
    emp_pdl::SepX3 sx;
    sx.C = C; sx.Cout = w.cout; sx.ks = ks;
    RC(dev_alloc(n, (size_t)ks * ks * C, &sx.dw));
    RC(launch_sepx3_pack_dw(dwi->second, ks, C, C, sx.dw, nullptr));
    RC(dev_alloc(n, (size_t)sepx3_pw_halfs(C, w.cout), &sx.pw));
    RC(launch_sepx3_pack_pw(w.w, C, C, w.cout, sx.pw, nullptr));
    n->sepx3[base] = sx;
  }
  EMP_CHECK_HIP(hipStreamSynchronize(nullptr));
  return EMP_OK;
}

// fp16x3 mode, round 6: the two decoders' low-level projections of stage i read the same encoder map: weights stacked along
// Cout, one launch with two destinations (conv16x3.hip store4) -- the widest map of the network is read once instead of twice
int x3_merged_projections(emp_pdl* n) {
  for (int i = 0; i < n->cfg.n_stages; ++i) {
    const std::string tail = ".project." + std::to_string(i) + ".0";
    auto ia = n->w32.find(kDecoders[0] + tail), ib = n->w32.find(kDecoders[1] + tail);
    if (ia == n->w32.end() || ib == n->w32.end()) continue;
    const emp_pdl::W32 &wa = ia->second, &wb = ib->second;
    if (wa.cin16 != wb.cin16 || wa.kh != 1 || wb.kh != 1 || wa.kw != 1 || wb.kw != 1 || wa.cout % 4 || wb.cout % 4 || wa.cin16 >= 1024) continue;
    emp_pdl::W32 m;
    RC(stack32(n, wa, wb, &m));
    n->w32["decoders" + tail] = m;
  }
  return EMP_OK;
}

// the plane region's layers: ResNet layer3 / layer4 and the ASPP convolutions
bool x3_region(const std::string& name) {
  return name.find("encoder.layer3.") == 0 || name.find("encoder.layer4.") == 0 || name.find(".aspp.") != std::string::npos;
}

// conv16x3p_kernel's packed hi / lo image of w
int x3p_image(emp_pdl* n, emp_pdl::W32& w, int64_t halfs) {
  RC(dev_alloc(n, (size_t)halfs, &w.wimgp));
  w.x3p_kg = x3p_kgroup(w.kh * w.kw, w.cin16);
  return launch_x3p_pack(w.w, w.wimgp, w.cout, w.kh * w.kw * w.cin16, nullptr, w.kh * w.kw, w.cin16, w.x3p_kg);
}

// fp16x3 mode: every convolution weight once more as fp16 pairs (hi | lo << 16, the fp32 blob's layout), so that the
// kernel's weight staging is a lane permutation instead of five vector operations per element (conv16x3.hip)
int x3_weight_images(emp_pdl* n) {
  for (auto& kv : n->w32) {
    emp_pdl::W32& w = kv.second;
    const int64_t cnt = (int64_t)w.cout * (w.kh * w.kw * w.cin16 + w.cin2_16);
    RC(dev_alloc(n, (size_t)(cnt > 0 ? cnt : 4), &w.wp));
    RC(launch_split_pairs(w.w, w.wp, cnt, nullptr));
    // long-K layers (the split-role kernel's): the weights once more as that kernel's LDS image, fetched by LDS-DMA
    const int K = w.kh * w.kw * w.cin16;
    const int64_t ih = (w.cin2_16 == 0 && K >= 1024) ? x3_weight_image_halfs(w.cout, K, w.cin16) : 0;
    if (ih > 0) {
      RC(dev_alloc(n, (size_t)ih, &w.wimg));
      RC(launch_x3_weight_image(w.w, w.wimg, w.cout, K, nullptr));
    }
    // round 6: the plane region's layers (Cout % 256 == 0, Cin % 32 == 0) once more as conv16x3p_kernel's packed hi / lo image
    const int64_t ip = (n->x3_planes && n->cfg.encoder == 0 && x3_region(kv.first) && w.cin2_16 == 0 && w.cin16 % 32 == 0 && K >= 128) ? x3p_image_halfs(w.cout, K) : 0;
    if (ip > 0) RC(x3p_image(n, w, ip));
  }
  return EMP_OK;
}

// the two decoders' ASPP branch i reads the same p5: [semantic ; instance] weights stacked along Cout, ONE launch with two
// destinations (twice the workgroups per launch: a batch of 8 tiles of 1024^2 fills the chip with the 256-channel branches)
int x3_merged_aspp(emp_pdl* n) {
  for (int i = 0; i <= 3; ++i) {
    const std::string tail = ".aspp.convs." + std::to_string(i) + ".0";
    auto ia = n->w32.find(kDecoders[0] + tail), ib = n->w32.find(kDecoders[1] + tail);
    if (ia == n->w32.end() || ib == n->w32.end()) continue;
    const emp_pdl::W32 &wa = ia->second, &wb = ib->second;
    if (!wa.wimgp || !wb.wimgp || wa.cout != wb.cout || wa.cin16 != wb.cin16 || wa.kh != wb.kh || wa.kw != wb.kw) continue;
    emp_pdl::W32 m;
    RC(stack32(n, wa, wb, &m));
    const int64_t ip = x3p_image_halfs(m.cout, m.kh * m.kw * m.cin16);
    if (ip <= 0) continue;
    RC(x3p_image(n, m, ip));
    n->w32["decoders" + tail] = m;
  }
  return EMP_OK;
}

// every layer of the plane region has its packed image, and no low-level skip leaves the region
bool x3_planes_complete(const emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  bool ok = true;
  for (auto& kv : n->w32) {
    const bool boundary = kv.first == "encoder.layer3.0.conv1" || kv.first == "encoder.layer3.0.downsample.0" || kv.first.find("conv3+ds") != std::string::npos;
    if (x3_region(kv.first) && !boundary && !kv.second.wimgp) ok = false;      // (the boundary layers read the fp32 layer2 map: round 5's kernels)
  }
  for (int i = 0; i < (c.arch == 0 ? c.n_stages : 0); ++i) ok = ok && c.low_level_stages[i] <= 2;      // a low-level skip out of the region would need a conversion
  return ok;
}

}  // namespace

namespace emp {

int finalize32(emp_pdl* n) {
  const emp_pdl_config& c = n->cfg;
  RC(pack32_encoder(n));
  RC(c.arch == 1 ? pack32_bifpn(n) : pack32_deeplab(n));
  RC(pack32_heads_pointrend(n));
  if (n->precision != 2) return EMP_OK;
  if (n->x3_ksplit && !n->x3_kpart) RC(dev_alloc(n, (size_t)X3_KPART_BYTES / sizeof(float), &n->x3_kpart));
  if (n->x3_fuse_sep) RC(x3_sep_weights(n));
  if (c.arch == 0 && c.ins_decoder && n->x3_merge_proj) RC(x3_merged_projections(n));
  RC(x3_weight_images(n));
  if (n->x3_planes && c.encoder == 0 && c.arch == 0 && c.ins_decoder && n->x3_merge_aspp) RC(x3_merged_aspp(n));
  EMP_CHECK_HIP(hipStreamSynchronize(nullptr));
  if (n->x3_planes && c.encoder == 0) n->x3_planes_ready = x3_planes_complete(n);
  return EMP_OK;
}

}  // namespace emp

namespace {

// out[:, :, :, out_coff : out_coff + Cout) = act(conv(in[:, :, :, in_coff : in_coff + Cin16)) + bias (+ bias_n) (+ res))
struct C32Opt {      // everything about a c32() launch beyond source, destination and stream
  int stride = 1, pad = 0, dil = 1, act = ACT_NONE;
  const T32* res = nullptr;               // residual added before the activation
  const float* bias_n = nullptr;          // per-image bias
  int ps_cout = 0;                        // pixel-shuffled output (the transposed convs): couts per sub-pixel
  int groups = 1;                         // grouped 3x3 of a RegNet block
  const float* head_w = nullptr;          // fp16x3: the head's 1x1 in the epilogue, partial sums per cout tile, head_c planes
  float* head_part = nullptr;
  int head_c = 0;
  const T32* in2 = nullptr;               // K-concatenated second source, sampled with stride2
  int stride2 = 1;
  const T32* out2 = nullptr;              // couts [split2, Cout) go here
  int out2_coff = 0, split2 = 0;
};

int c32(emp_pdl* n, const std::string& wname, const T32& in, int in_coff, const T32& out, int out_coff, hipStream_t s,
        const C32Opt& o = {}) {
  const auto& [stride, pad, dil, act, res, bias_n, ps_cout, groups, head_w, head_part, head_c, in2, stride2, out2, out2_coff, split2] = o;      // (C32Opt's members, in its order)
  const emp_pdl::W32& w = n->w32.at(wname);
  Conv32 p{};
  if (out2) {      // couts [split2, Cout) -> out2 (the merged ASPP branches on conv16x3p; the merged low-level projections on conv16x3's vector epilogue)
    EMP_REQUIRE(n->precision == 2 && out2->fmt == out.fmt && (!out2->fmt || out2_coff % 32 == 0) && (in.fmt || !out.fmt), "%s: bad second destination", wname.c_str());
    p.out2 = out2->p + out2_coff; p.out2_ld = out2->ld; p.split2 = split2;
  }
  if (groups > 1) {      // grouped 3x3 of a RegNet block: w.cin is the group width, w.cout all output channels
    EMP_REQUIRE(w.cout % groups == 0 && in_coff == 0 && out_coff == 0 && !res && !bias_n && !ps_cout, "%s (fp32): bad grouped call",
                wname.c_str());
    p.groups = groups;
    p.cin_g = w.cin;
  }
  // an hl32 map (T32::fmt, the fp16x3 mode's plane region): halfs, channel c of a row at (c / 32) * 64 + c % 32 -- a channel
  // slice starts at a multiple of 32 channels = coff * 2 halfs = coff floats into the row
  EMP_REQUIRE((!in.fmt || in_coff % 32 == 0) && (!out.fmt || out_coff % 32 == 0), "%s: hl32 channel slices start at multiples of 32", wname.c_str());
  EMP_REQUIRE(!in.fmt || (w.wimgp && groups <= 1 && !in2 && !head_w && !ps_cout), "%s: an hl32 input needs the packed image of a plain convolution", wname.c_str());
  p.in = in.p + in_coff; p.in_ld = in.ld; p.in_fmt = in.fmt;
  p.wimgp = in.fmt ? w.wimgp : nullptr;
  p.x3p_kg = w.x3p_kg;
  p.w = w.w; p.bias = w.b; p.bias_n = bias_n;
  p.res = res ? res->p : nullptr; p.res_ld = res ? res->ld : 0; p.res_fmt = res ? res->fmt : 0;
  p.out = out.p + out_coff; p.out_ld = out.ld; p.out_fmt = out.fmt;
  p.N = in.N; p.H = in.H; p.W = in.W; p.Cin = w.cin16; p.Cout = w.cout / groups; p.KH = w.kh; p.KW = w.kw;
  p.stride = stride; p.pad = pad; p.dil = dil;
  p.Ho = (in.H + 2 * pad - dil * (w.kh - 1) - 1) / stride + 1;
  p.Wo = (in.W + 2 * pad - dil * (w.kw - 1) - 1) / stride + 1;
  p.act = act; p.ps_cout = ps_cout;
  p.x3 = n->precision == 2;
  p.wpair = p.x3 ? w.wp : nullptr;
  p.wimg = (p.x3 && groups <= 1) ? w.wimg : nullptr;
  p.head_w = head_w; p.head_part = head_part; p.head_c = head_c;      // (fp16x3 only: the map `out` is then not written)
  if (p.x3 && n->x3_ksplit && n->x3_kpart && !head_w && !in2 && (in.fmt || !out2)) { p.kpart = n->x3_kpart; p.kpart_bytes = X3_KPART_BYTES; }
  if (in2) {      // K-concatenated second source (fp16x3 only: weights packed by pack32_conv3_ds)
    EMP_REQUIRE(p.x3 && w.cin2_16 > 0 && w.cin2_16 <= in2->ld && in2->N == in.N, "%s: second source mismatch", wname.c_str());
    p.in2 = in2->p; p.in2_ld = in2->ld; p.Cin2 = w.cin2_16; p.H2 = in2->H; p.W2 = in2->W; p.stride2 = stride2;
    n->flops += 2.0 * (double)p.N * p.Ho * p.Wo * w.cout * (double)w.cin2;
  } else {
    EMP_REQUIRE(w.cin2_16 == 0, "%s: packed for two sources", wname.c_str());
  }
  EMP_REQUIRE(!head_w || p.x3, "%s: the fused head exists in the fp16x3 mode only", wname.c_str());
  const int up = ps_cout ? 2 : 1;
  EMP_REQUIRE(p.Ho * up == out.H && p.Wo * up == out.W && in.N == out.N, "%s (fp32): output shape mismatch", wname.c_str());
  EMP_REQUIRE(in_coff + (groups - 1) * w.cin + w.cin16 <= in.ld && out_coff + (ps_cout ? ps_cout : (out2 ? split2 : w.cout)) <= out.ld,
              "%s (fp32): channel slice out of range (needs %d of a row of %d)", wname.c_str(), in_coff + (groups - 1) * w.cin + w.cin16, in.ld);
  n->flops += 2.0 * (double)p.N * p.Ho * p.Wo * w.cout * (double)(w.cin * w.kh * w.kw);
  if (n->profile && p.x3 && p.in_fmt) {     // emp_pdl_profile: HIP events around the plane region's launches (the fp16x3 mode's dominant kernel)
    // (booked at the fp16 MFMA flops: three products per MAC)
    return profiled_launch(n, s, 3.0 * 2.0 * (double)p.N * p.Ho * p.Wo * w.cout * (double)(w.cin16 * w.kh * w.kw), [&] { return launch_conv32(p, s); });
  }
  return launch_conv32(p, s);
}

// One forward of the fp32 / fp16x3 graph: the maps made so far by name, and what its stages share
struct Fwd32 : Forward {
  bool hlr;      // fp16x3 mode, round 6: layer3 / layer4 / ASPP maps as hl32 planes on conv16x3p_kernel (emp_pdl members x3_planes*)
  std::map<std::string, T32> T;
  std::string x;

  T32& A(const std::string& k) { return T.at(k); }
  int mk(const std::string& k, int H_, int W_, int C_, int fmt = 0) {
    T32 t;
    int rc = t32(n, k, N, H_, W_, C_, &t);
    t.fmt = fmt;
    T[k] = t;
    if (!rc) note32(n, k, "map", t.p, N, H_, W_, C_, t.ld, fmt);
    return rc;
  }
  int mkp(const std::string& k, int H_, int W_, int C_);
  int sep(const std::string& base, const T32& in, int ks, int act, const std::string& dwkey, const T32* out, const float* hw,
          const float* hb, int hcn, float* hout, bool* fused);
  int regnet_encoder();
  int resnet_encoder();
  int bifpn_decoders();
  int merged_aspp(const T32& src, int fmt);
  int deeplab_decoders();
  int heads();
  int pointrend();
};

// A RegNet map.  RegNet's widths are multiples of 8, not of 16: every map gets a row of round_up(C, 16) + 16
// floats whose tail stays zero (buf32 clears a buffer when it allocates it and no kernel writes beyond C), so that a
// consumer reading its input channels padded to 16 -- from a group's first channel, in the grouped 3x3 -- stays
// inside the row and meets zeros (or the next group's finite values) under zero weights.
int Fwd32::mkp(const std::string& k, int H_, int W_, int C_) {
  T32 t;
  t.N = N; t.H = H_; t.W = W_; t.C = C_; t.ld = round_up(C_, 16) + 16;
  const size_t had = n->pool32.count(k) ? n->pool32[k].second : 0;
  const int rc = buf32(n, k, (size_t)N * H_ * W_ * t.ld, &t.p);
  if (rc) return rc;
  // a buffer kept from a forward of another shape holds that forward's values where this one's row tails are
  const std::array<int, 4> geo = {N, H_, W_, t.ld};
  auto gi = n->geom32.find(k);
  if (gi == n->geom32.end() || gi->second != geo) {
    if (had >= (size_t)N * H_ * W_ * t.ld && gi != n->geom32.end())
      EMP_CHECK_HIP(hipMemsetAsync(t.p, 0, (size_t)N * H_ * W_ * t.ld * sizeof(float), s));
    n->geom32[k] = geo;
  }
  T[k] = t;
  note32(n, k, "map", t.p, N, H_, W_, C_, t.ld);
  return EMP_OK;
}

// The separable block `base` ("... .sepconv": depthwise ks x ks -> pointwise -> act [-> a head's 1x1]) of `in`.  fp16x3 mode: ONE launch
// where the fused kernel takes it (sepconv_x3.hip; at a head, out == nullptr, hw / hb / hcn -> hout and no map).  Else the depthwise
// launch into the buffer `dwkey` -- made on this path only -- and, where there is an output map, the pointwise conv; *fused tells a
// head whether its pointwise half is still to run
int Fwd32::sep(const std::string& base, const T32& in, int ks, int act, const std::string& dwkey, const T32* out, const float* hw,
               const float* hb, int hcn, float* hout, bool* fused) {
  auto it = n->sepx3.find(base);
  const int64_t tiles = (int64_t)N * ((in.H + 7) / 8) * ((in.W + 15) / 16);
  *fused = n->precision == 2 && it != n->sepx3.end() && !in.fmt && in.ld >= it->second.C && tiles >= n->x3_sep_min_tiles &&
           sepconv_x3_supported(it->second.C, it->second.Cout, hcn, it->second.ks);
  if (*fused) {
    const emp_pdl::SepX3& sx = it->second;
    n->flops += 2.0 * sx.ks * sx.ks * (double)N * in.H * in.W * in.C + 2.0 * (double)N * in.H * in.W * sx.Cout * (double)n->w32.at(base + ".1").cin;
    return launch_sepconv_x3(in.p, N, in.H, in.W, sx.C, in.ld, sx.dw, sx.pw, n->w32.at(base + ".1").b, sx.Cout, act, out ? out->p : nullptr,
                             out ? out->ld : 0, hw, hb, hcn, hout, (int64_t)in.H * in.W, s, sx.ks);
  }
  RC(mk(dwkey, in.H, in.W, in.C));
  n->flops += 2.0 * ks * ks * (double)N * in.H * in.W * in.C;
  RC(launch_dwconv_f32(in.p, N, in.H, in.W, in.C, in.ld, n->f32w.at(base + ".0.dw32"), ks, A(dwkey).p, A(dwkey).ld, s));
  return out ? c32(n, base + ".1", A(dwkey), 0, *out, 0, s, {.act = act}) : EMP_OK;
}

// RegNet (regnet.py:160-166)
int Fwd32::regnet_encoder() {
  RC(mkp("stem", H / 2, W / 2, c.rn_stem));
  RC(launch_stem3x3s2_f32(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("rn.stem.w"), n->f32w.at("rn.stem.b"), c.rn_stem,
                            A("stem").p, A("stem").ld, s));
  n->flops += 2.0 * N * (H / 2) * (W / 2) * (double)c.rn_stem * 9.0;
  x = "stem";
  pyr[0] = "stem";
  for (const RegBlock& k : n->reg_blocks) {
    const std::string& p = k.name;
    const int w = k.width, g = k.groups, sb = k.stride;
    const T32 xin = A(x);
    const int ho = (xin.H - 1) / sb + 1, wo = (xin.W - 1) / sb + 1;
    RC(mkp(p + ".a", xin.H, xin.W, w));
    RC(c32(n, p + ".bottleneck.a.0", xin, 0, A(p + ".a"), 0, s, {.act = ACT_RELU}));
    RC(mkp(p + ".b", ho, wo, w));
    RC(c32(n, p + ".bottleneck.b.0", A(p + ".a"), 0, A(p + ".b"), 0, s, {.stride = sb, .pad = 1, .act = ACT_RELU, .groups = g}));
    if (c.rn_se) {      // per-pixel gate: x * sigmoid(W2 relu(W1 x)) (blocks.py:35-50: the pool is 1 x 1)
      RC(mkp(p + ".se1", ho, wo, w / 4));
      RC(c32(n, p + ".bottleneck.se.se.0", A(p + ".b"), 0, A(p + ".se1"), 0, s, {.act = ACT_RELU}));
      RC(mkp(p + ".se2", ho, wo, w));
      RC(c32(n, p + ".bottleneck.se.se.2", A(p + ".se1"), 0, A(p + ".se2"), 0, s));
      RC(launch_gate_mul_f32(A(p + ".b").p, A(p + ".b").ld, A(p + ".se2").p, A(p + ".se2").ld, (int64_t)N * ho * wo, w, s));
    }
    const T32* idn = &A(x);
    if (k.shortcut) {
      RC(mkp(p + ".ds", ho, wo, w));
      RC(c32(n, p + ".downsample.conv.0", xin, 0, A(p + ".ds"), 0, s, {.stride = sb}));
      idn = &A(p + ".ds");
    }
    RC(mkp(p, ho, wo, w));
    RC(c32(n, p + ".bottleneck.c.0", A(p + ".b"), 0, A(p), 0, s, {.act = ACT_RELU, .res = idn}));
    x = p;
    if (k.last) pyr[k.si] = p;
  }
  return EMP_OK;
}

int Fwd32::resnet_encoder() {
  n->flops += 2.0 * N * (H / 2) * (W / 2) * 64.0 * 49.0;
  RC(mk("p1", H / 4, W / 4, 64));
  if (n->precision == 2 && n->x3_fuse_stem) {
    // fp16x3 mode, round 6: conv1 + bn1 + relu + maxpool as one launch on the matrix pipe (stem.hip stem_pool32_kernel: the three-MFMA
    // split product of every other convolution of the mode, fp32 tile and output); the half-resolution map is never written
    RC(launch_stem_pool_f32(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("stem.w"), n->f32w.at("stem.b"), A("p1").p, s));
  } else {
    RC(mk("stem", H / 2, W / 2, 64));
    RC(launch_stem7x7_f32(img, dtype, sub, mul, N, H, W, vh, vw, n->f32w.at("stem.w"), n->f32w.at("stem.b"), A("stem").p, s));
    RC(launch_maxpool3x3s2_f32(A("stem").p, N, H / 2, W / 2, 64, A("p1").p, s));
  }
  x = "p1";
  pyr[0] = "p1";
  for (const ResBlock& k : n->res_blocks) {
    const std::string& p = k.name;
    const int sb = k.stride, dil = k.dil, planes = k.planes;
    const T32 xin = A(x);
    const int ho = (xin.H - 1) / sb + 1, wo = (xin.W - 1) / sb + 1;
    // plane region (li >= 3): every map hl32 except where round 5's kernels still read it -- layer3.0's conv1 and
    // conv3 + shortcut take the fp32 layer2 map (and the fp32 c2) and WRITE hl32 (Conv32::out_fmt)
    const int pl = (hlr && k.li >= 3) ? 1 : 0;
    const bool fuse_ds = k.b == 0 && n->precision == 2 && n->x3_fuse_ds && !(pl && xin.fmt);
    RC(mk(p + ".c1", xin.H, xin.W, planes, pl));
    RC(c32(n, p + ".conv1", xin, 0, A(p + ".c1"), 0, s, {.act = ACT_RELU}));
    RC(mk(p + ".c2", ho, wo, planes, (pl && !fuse_ds) ? 1 : 0));
    RC(c32(n, p + ".conv2", A(p + ".c1"), 0, A(p + ".c2"), 0, s, {.stride = sb, .pad = dil, .dil = dil, .act = ACT_RELU}));
    RC(mk(p, ho, wo, planes * 4, pl));
    if (fuse_ds) {
      // fp16x3 mode: relu(conv3(c2) + downsample(x)) as one convolution over the concatenated K (the shortcut map is
      // neither written nor read back)
      RC(c32(n, p + ".conv3+ds", A(p + ".c2"), 0, A(p), 0, s, {.act = ACT_RELU, .in2 = &xin, .stride2 = sb}));
    } else {
      const T32* idn = &A(x);
      if (k.b == 0) {
        RC(mk(p + ".ds", ho, wo, planes * 4, pl));
        RC(c32(n, p + ".downsample.0", xin, 0, A(p + ".ds"), 0, s, {.stride = sb}));
        idn = &A(p + ".ds");
      }
      RC(c32(n, p + ".conv3", A(p + ".c2"), 0, A(p), 0, s, {.act = ACT_RELU, .res = idn}));
    }
    x = p;
    if (k.last) pyr[k.li] = p;
  }
  if (hlr && c.arch == 1) {
    // the BiFPN reads P4 / P5 with round 5's kernels (128-channel nodes): fp32 copies of the two pyramid levels
    for (int li = 3; li <= 4; ++li) {
      const T32 src = A(pyr[li]);
      const std::string k = pyr[li] + ".f32";
      RC(mk(k, src.H, src.W, src.C));
      RC(launch_hl32_to_f32(reinterpret_cast<const half_t*>(src.p), A(k).p, (int64_t)N * src.H * src.W, src.C, src.ld, src.C, s));
      pyr[li] = k;
    }
  }
  return EMP_OK;
}

// ---- BiFPN decoders (bifpn.py:185-236) ----
int Fwd32::bifpn_decoders() {
  const int F = c.fpn_dim;
  const T32 p2 = A(pyr[1]);
  RC(mk("p2f", p2.H, p2.W, F));
  RC(c32(n, "p2_resample.conv.0", p2, 0, A("p2f"), 0, s));
  auto resample = [&](const std::string& rk, const std::string& src, const std::string& dst, std::string* name) -> int {
    *name = src;
    if (!n->w32.count(rk)) return EMP_OK;
    const T32 in = A(src);
    RC(mk(dst, in.H, in.W, F));
    *name = dst;
    return c32(n, rk, in, 0, A(dst), 0, s);
  };
  auto node = [&](const std::string& dirpre, const std::string& q, const std::string& a, const std::string& b2, const std::string& c3,
                  float ca, float cb, float cc, int mode, const std::string& outname) -> int {
    const T32 tb = A(b2);      // the node's size: its (resampled) input of this level
    const float *pa = A(a).p, *pc = c3.empty() ? nullptr : A(c3).p;
    const std::string fz = q + (mode ? ".bun.fz" : ".tdn.fz");
    RC(mk(fz, tb.H, tb.W, F));
    RC(launch_fuse_combine_f32(pa, tb.p, pc, ca, cb, cc, mode, N, tb.H, tb.W, F, A(fz).p, s));
    bool fused = false;
    RC(mk(outname, tb.H, tb.W, F));
    return sep(dirpre + ".after_combines.0.0.sepconv", A(fz), 3, ACT_SILU, q + (mode ? ".bun.dw" : ".tdn.dw"), &A(outname), nullptr, nullptr, 0,
               nullptr, &fused);
  };
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    const std::string fp = std::string(kBifpn[d]) + "_fpn";
    const T32 p5 = A(pyr[4]);
    RC(mk(fp + ".p6pre", p5.H, p5.W, F));
    RC(c32(n, fp + ".p6_resample.conv.0", p5, 0, A(fp + ".p6pre"), 0, s));
    RC(mk(fp + ".in.P6", p5.H / 2, p5.W / 2, F));
    RC(launch_maxpool3x3s2_f32(A(fp + ".p6pre").p, N, p5.H, p5.W, F, A(fp + ".in.P6").p, s));
    RC(mk(fp + ".in.P7", p5.H / 4, p5.W / 4, F));
    RC(launch_maxpool3x3s2_f32(A(fp + ".in.P6").p, N, p5.H / 2, p5.W / 2, F, A(fp + ".in.P7").p, s));
    std::string feat[5] = {pyr[2], pyr[3], pyr[4], fp + ".in.P6", fp + ".in.P7"};
    for (int li = 0; li < c.fpn_layers; ++li)
      RC(bifpn_layer(n, fp + ".bifpns." + std::to_string(li), fp + ".l" + std::to_string(li), feat, resample, node));
    const std::string dp = std::string(kBifpn[d]) + "_decoder";
    const std::string skips[5] = {feat[3], feat[2], feat[1], feat[0], "p2f"};
    std::string xx = feat[4];
    for (int i = 0; i < 5; ++i) {
      const T32 in = A(xx);
      const std::string cn = dp + ".cat" + std::to_string(i);
      RC(mk(cn, in.H * 2, in.W * 2, 2 * F));
      RC(c32(n, dp + ".upsamplings." + std::to_string(i) + ".0", in, 0, A(cn), 0, s, {.act = ACT_RELU, .ps_cout = F}));
      const T32 sk = A(skips[i]);
      RC(launch_bilinear_ac_f32_nhwc(sk.p, N, sk.H, sk.W, F, sk.ld, A(cn).p + F, sk.H, sk.W, 2 * F, s));      // same size: copy
      xx = cn;
    }
    const T32 cat = A(xx);
    RC(mk(dp + ".out", cat.H, cat.W, F));
    bool fused = false;
    RC(sep(dp + ".fusion.0.sepconv", cat, 5, ACT_RELU, dp + ".dw", &A(dp + ".out"), nullptr, nullptr, 0, nullptr, &fused));
    dec_out[d] = dp + ".out";
  }
  return EMP_OK;
}

// ASPP branch i of BOTH decoders as one launch on the plane kernel (weights stacked along Cout at finalize, two destinations): src is p5
// as an hl32 map, the concat buffers are made in format fmt
int Fwd32::merged_aspp(const T32& src, int fmt) {
  for (int d = 0; d < 2; ++d) RC(mk(std::string(kDecoders[d]) + ".aspp.cat", src.H, src.W, 4 * n->aspp_ch, fmt));
  const T32 &c0 = A(std::string(kDecoders[0]) + ".aspp.cat"), &c1 = A(std::string(kDecoders[1]) + ".aspp.cat");
  for (int i = 0; i <= 3; ++i) {
    const int r = i ? c.atrous_rates[i - 1] : 1;
    RC(c32(n, "decoders.aspp.convs." + std::to_string(i) + ".0", src, 0, c0, i * n->aspp_ch, s,
        {.pad = i ? r : 0, .dil = r, .act = ACT_RELU, .out2 = &c1, .out2_coff = i * n->aspp_ch, .split2 = n->aspp_ch}));
  }
  return EMP_OK;
}

// ---- Panoptic-DeepLab decoders (decoders/panoptic_deeplab.py:68-80, aspp.py:96-102) ----
int Fwd32::deeplab_decoders() {
  const T32 p5 = A(pyr[4]);
  float* pooled;
  RC(buf32(n, "pooled", (size_t)N * p5.C, &pooled));
  note32(n, "pooled", "pooled", pooled, N, 1, 1, p5.C, p5.C);
  if (p5.fmt) RC(launch_avgpool_hl32(reinterpret_cast<const half_t*>(p5.p), N, p5.H * p5.W, p5.C, p5.ld, pooled, s));
  else RC(launch_avgpool_f32(p5.p, N, p5.H * p5.W, p5.C, p5.ld, pooled, s));
  // plane region: the ASPP branches of both decoders merged, from the hl32 p5 into hl32 concat buffers
  const bool have_merged = c.ins_decoder && n->w32.count("decoders.aspp.convs.0.0") && n->w32.count("decoders.aspp.convs.3.0");
  const bool merged = p5.fmt && have_merged;
  // below the plane region's threshold (small batches; round 6, late): the branches still run merged on the plane kernel -- K-split
  // (Conv32::kpart: 32 workgroups x 8 splits for ONE 1024^2 tile) -- from an hl32 copy of p5, into fp32 concat buffers
  const bool small = !p5.fmt && n->precision == 2 && n->x3_planes_ready && n->x3_ksplit && n->x3_small_aspp && n->x3_kpart && have_merged &&
                     p5.C % 32 == 0;
  if (small) {
    RC(mk("p5.hl32", p5.H, p5.W, p5.C, 1));
    const T32& ph = A("p5.hl32");
    RC(launch_hl32_from_f32(p5.p, reinterpret_cast<half_t*>(ph.p), (int64_t)N * p5.H * p5.W, p5.C, p5.ld, ph.ld, s));
    RC(merged_aspp(ph, 0));
  }
  if (merged) RC(merged_aspp(p5, 1));
  // the decoders' low-level projections, both decoders in one launch where finalize32 stacked their weights: the .cat buffers of
  // both decoders exist before the loop below fills their up-sampled halves
  bool proj_done[3] = {false, false, false};
  if (n->precision == 2 && c.ins_decoder) {
    int xch0 = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const std::string wn = "decoders.project." + std::to_string(i) + ".0";
      if (n->w32.count(wn)) {
        const T32 low = A(pyr[c.low_level_stages[i]]);
        const int cps = round_up(xch0 + c.low_level_proj_sem[i], 32), cpi = round_up(xch0 + c.low_level_proj_ins[i], 32);
        const std::string qs = std::string(kDecoders[0]) + ".stage" + std::to_string(i), qi = std::string(kDecoders[1]) + ".stage" + std::to_string(i);
        RC(mk(qs + ".cat", low.H, low.W, cps));
        RC(mk(qi + ".cat", low.H, low.W, cpi));
        if (!low.fmt && xch0 % 4 == 0) {
          RC(c32(n, wn, low, 0, A(qs + ".cat"), xch0, s,
              {.act = ACT_RELU, .out2 = &A(qi + ".cat"), .out2_coff = xch0, .split2 = c.low_level_proj_sem[i]}));
          proj_done[i] = true;
        }
      }
      xch0 = n->dec_ch;
    }
  }
  for (int d = 0; d < (c.ins_decoder ? 2 : 1); ++d) {
    const std::string p = kDecoders[d];
    float *poolfeat, *bias_n;
    RC(buf32(n, p + ".poolfeat", (size_t)N * n->aspp_ch, &poolfeat));
    RC(buf32(n, p + ".bias_n", (size_t)N * n->aspp_ch, &bias_n));
    note32(n, p + ".poolfeat", "poolfeat", poolfeat, N, 1, 1, n->aspp_ch, n->aspp_ch);
    note32(n, p + ".bias_n", "bias_n", bias_n, N, 1, 1, n->aspp_ch, n->aspp_ch);
    RC(launch_gemv(pooled, N, p5.C, n->f32w.at(p + ".pool.w"), nullptr, n->aspp_ch, 1, poolfeat, s));
    RC(launch_gemv(poolfeat, N, n->aspp_ch, n->f32w.at(p + ".projpool.w"), nullptr, n->aspp_ch, 0, bias_n, s));
    if (!merged && !small) {
      RC(mk(p + ".aspp.cat", p5.H, p5.W, 4 * n->aspp_ch, p5.fmt));      // (the projection reads it as it was written; its output is fp32: the up-sampler's input)
      RC(c32(n, p + ".aspp.convs.0.0", p5, 0, A(p + ".aspp.cat"), 0, s, {.act = ACT_RELU}));
      for (int i = 1; i <= 3; ++i) {
        const int r = c.atrous_rates[i - 1];
        RC(c32(n, p + ".aspp.convs." + std::to_string(i) + ".0", p5, 0, A(p + ".aspp.cat"), i * n->aspp_ch, s,
            {.pad = r, .dil = r, .act = ACT_RELU}));
      }
    }
    RC(mk(p + ".aspp", p5.H, p5.W, n->aspp_ch));
    RC(c32(n, p + ".aspp.project.0", A(p + ".aspp.cat"), 0, A(p + ".aspp"), 0, s, {.act = ACT_RELU, .bias_n = bias_n}));
    std::string xx = p + ".aspp";
    int xch = n->aspp_ch;
    for (int i = 0; i < c.n_stages; ++i) {
      const T32 low = A(pyr[c.low_level_stages[i]]);
      const int lp = d == 0 ? c.low_level_proj_sem[i] : c.low_level_proj_ins[i];
      const int cpad = round_up(xch + lp, n->precision == 2 ? 32 : 16);      // (finalize32 packed the block's weights for this width)
      const std::string q = p + ".stage" + std::to_string(i);
      RC(mk(q + ".cat", low.H, low.W, cpad));
      const T32 xa = A(xx);
      RC(launch_bilinear_ac_f32_nhwc(xa.p, N, xa.H, xa.W, xch, xa.ld, A(q + ".cat").p, low.H, low.W, cpad, s));
      if (!proj_done[i]) RC(c32(n, p + ".project." + std::to_string(i) + ".0", low, 0, A(q + ".cat"), xch, s, {.act = ACT_RELU}));
      RC(mk(q + ".out", low.H, low.W, n->dec_ch));
      bool fused = false;
      RC(sep(p + ".fuse." + std::to_string(i) + ".0.sepconv", A(q + ".cat"), 5, ACT_RELU, q + ".dw", &A(q + ".out"), nullptr, nullptr, 0, nullptr, &fused));
      xx = q + ".out";
      xch = n->dec_ch;
    }
    dec_out[d] = xx;
  }
  return EMP_OK;
}

// ---- heads (heads.py:12-19) ----
int Fwd32::heads() {
  const T32 semx = A(dec_out[0]), insx = A(dec_out[1]);
  const int hq = semx.H, wq = semx.W;
  EMP_REQUIRE(hq * 4 == H && wq * 4 == W, "the decoder output must be at 1/4 resolution (got %dx%d)", hq, wq);
  for (int k = 0; k < 3; ++k) {
    const std::string p = kHeads[k];
    const int hc = head_planes(n, k);
    const T32& xin = k == 0 ? semx : insx;
    float* dst;
    RC(buf32(n, p + ".out", (size_t)N * hc * hq * wq, &dst));
    if (k == 1 && !interp) dst = o_ctr;
    if (k == 2 && !interp) dst = o_off;
    head_out[k] = dst;
    note32(n, p + ".out", "out", dst, N, hq, wq, hc, hc);      // (where the forward wrote the head: the caller's tensor without interpolate_ins)
    // fp16x3 mode, round 6: depthwise + pointwise + ReLU + the head's 1x1 in one launch (sepconv_x3.hip, head_c <= 2); else the depthwise half
    bool fused = false;
    RC(sep(p + ".head.0.0.sepconv", xin, 5, ACT_RELU, p + ".dw", nullptr, n->f32w.at(p + ".head.1.w"), n->f32w.at(p + ".head.1.b"), hc, dst, &fused));
    if (fused) {
      n->flops += 2.0 * (double)N * hq * wq * n->dec_ch * hc;
      continue;
    }
    if (n->precision == 2 && n->x3_fuse_head && hc <= 4) {
      // fp16x3 mode: the head's 1x1 inside the pointwise conv's epilogue (conv16x3.hip HEAD): the dec_ch-wide map is
      // neither written nor read back; every cout tile leaves per-pixel partial sums, added in ascending order
      const int tiles = conv16x3_cout_tiles(n->dec_ch);
      float* part;
      RC(buf32(n, p + ".part", (size_t)tiles * N * hq * wq * hc, &part));
      note32(n, p + ".part", "part", part, N, hq, wq, hc, tiles);
      RC(c32(n, p + ".head.0.0.sepconv.1", A(p + ".dw"), 0, A(p + ".dw"), 0, s,
          {.act = ACT_RELU, .head_w = n->f32w.at(p + ".head.1.w"), .head_part = part, .head_c = hc}));
      RC(launch_head_finish_f32(part, tiles, N, hq * wq, hc, n->f32w.at(p + ".head.1.b"), dst, s));
    } else {
      RC(mk(p + ".pw", hq, wq, n->dec_ch));
      RC(c32(n, p + ".head.0.0.sepconv.1", A(p + ".dw"), 0, A(p + ".pw"), 0, s, {.act = ACT_RELU}));
      RC(launch_head1x1_f32(A(p + ".pw").p, N, hq * wq, n->dec_ch, n->dec_ch, n->f32w.at(p + ".head.1.w"), n->f32w.at(p + ".head.1.b"),
                              hc, dst, (int64_t)hq * wq, nullptr, s));
    }
    n->flops += 2.0 * (double)N * hq * wq * n->dec_ch * hc;
  }
  if (interp) {
    RC(launch_bilinear_ac_f32_nchw(head_out[1], N * 1, hq, wq, o_ctr, 4, s));
    RC(launch_bilinear_ac_f32_nchw(head_out[2], N * 2, hq, wq, o_off, 4, s));
  }
  return EMP_OK;
}

// ---- PointRend subdivision (point_rend.py:241-269, eval) ----
int Fwd32::pointrend() {
  const T32 semx = A(dec_out[0]);
  const int hq = semx.H, wq = semx.W;
  const int P = c.subdivision_num_points;
  const int ldp = round_up(n->dec_ch + n->ncls, 16);
  const float* coarse = head_out[0];
  const float* cur = coarse;
  int hh = hq, ww = wq;
  int64_t plane_max = (int64_t)hq * wq;
  for (int st = 0; st < RS; ++st) plane_max *= 4;
  float* fkeys;
  RC(buf32(n, "pr.keys", (size_t)N * plane_max, &fkeys));
  note32(n, "pr.keys", "pr.keys", fkeys, N, 1, plane_max, 1, 1);
  float* ftopk;
  const size_t topk_bytes = topk_work_bytes(N, plane_max);
  RC(buf32(n, "pr.topk", (topk_bytes + 3) / 4, &ftopk));
  note32(n, "pr.topk", "pr.topk", ftopk, 1, 1, (int64_t)((topk_bytes + 3) / 4), 1, 1);
  float* fidx;
  RC(buf32(n, "pr.idx", (size_t)N * P, &fidx));
  note32(n, "pr.idx", "pr.idx", fidx, N, 1, P, 1, 1);
  T32 X[2];
  for (int j = 0; j < 2; ++j) {
    X[j].N = 1; X[j].H = 1; X[j].W = N * P; X[j].C = ldp; X[j].ld = ldp;
    RC(buf32(n, j ? "pr.x1" : "pr.x0", (size_t)N * P * ldp, &X[j].p));
    note32(n, j ? "pr.x1" : "pr.x0", "pr.x", X[j].p, 1, 1, (int64_t)N * P, ldp, ldp);
  }
  for (int st = 0; st < RS; ++st) {
    float* nxt = o_sem;
    if (st + 1 < RS) {
      RC(buf32(n, "pr.sem" + std::to_string(st), (size_t)N * n->ncls * hh * ww * 4, &nxt));
      note32(n, "pr.sem" + std::to_string(st), "pr.sem", nxt, N, hh * 2, ww * 2, n->ncls, n->ncls);
    }
    RC(launch_upsample2x_keys(cur, N, n->ncls, hh, ww, nxt, (uint32_t*)fkeys, s));
    hh *= 2; ww *= 2;
    const int64_t plane = (int64_t)hh * ww;
    const int k = (int)(plane < P ? plane : P);
    RC(launch_topk_smallest((const uint32_t*)fkeys, N, plane, k, (char*)ftopk, topk_bytes, (int32_t*)fidx, s));
    RC(launch_point_features_f32(semx.p, N, hq, wq, n->dec_ch, semx.ld, coarse, n->ncls, (const int32_t*)fidx, k, hh, ww, X[0].p,
                                   X[1].p, ldp, s));
    T32 xa[2] = {X[0], X[1]};
    xa[0].W = xa[1].W = N * k;
    int curx = 0;
    for (int f = 0; f < c.num_fc; ++f) {
      RC(c32(n, "semantic_pr.point_head.fc_layers." + std::to_string(f) + ".0", xa[curx], 0, xa[curx ^ 1], 0, s, {.act = ACT_RELU}));
      curx ^= 1;
    }
    RC(launch_head1x1_f32(xa[curx].p, N, k, ldp, ldp, n->f32w.at("pr.predictor.w32"), n->f32w.at("pr.predictor.b"), n->ncls, nxt,
                            plane, (const int32_t*)fidx, s));
    n->flops += 2.0 * (double)N * k * ldp * n->ncls;
    cur = nxt;
  }
  return EMP_OK;
}

}  // namespace

namespace emp {

int run32(emp_pdl* n, const void* img, int dtype, float sub, float mul, int N, int H, int W, int vh, int vw, int RS, int interp,
          float* o_sem, float* o_ctr, float* o_off, hipStream_t s) {
  const emp_pdl_config& c = n->cfg;
  EMP_REQUIRE(N > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "forward: H=%d W=%d must be positive multiples of 16", H, W);
  EMP_REQUIRE(RS >= 1 && RS <= 6, "render_steps=%d out of range", RS);
  EMP_REQUIRE(c.arch == 0 || (H % 128 == 0 && W % 128 == 0), "BiFPN forward: H=%d W=%d must be multiples of 128", H, W);
  n->flops = 0.0;
  n->maps32.clear();
  n->maps32_at.clear();
  // (an encoder at output stride 32 -- the BiFPN networks -- has a quarter of those tiles in layer4: BiFPN-PR with the region on / off
  //  492 / 513 tiles/s at batch 8, 594 / 581 at 16, 651 / 631 at 32: its threshold is twice the stride-16 one)
  const bool hlr = n->precision == 2 && n->x3_planes_ready && c.encoder == 0 &&
                   ((int64_t)N * (H / 16) * (W / 16)) / 256 >= n->x3_planes_min_tiles * (c.stage4_stride == 32 ? 2 : 1);
  Fwd32 f{{n, c, img, dtype, sub, mul, N, H, W, vh, vw, RS, interp, o_sem, o_ctr, o_off, s}, hlr};
  RC(c.encoder == 1 ? f.regnet_encoder() : f.resnet_encoder());
  RC(c.arch == 1 ? f.bifpn_decoders() : f.deeplab_decoders());
  if (!c.ins_decoder) f.dec_out[1] = f.dec_out[0];
  RC(f.heads());
  return f.pointrend();
}

}  // namespace emp
