// C ABI of the ResNet-152 res5c feature extractor (include/n2nmn.h section 10): the n2nmn_resnet handle, its
// folded-weight store, the bottleneck schedule and the buffer plan.  Host code only;
// kernels: kernels_resnet.hip and, for every 3x3, kernels_vgg.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/n2nmn.h"
#include "kernels.h"
#include "resnet_kernels.h"

#include "ctx.h"

using namespace n2nmn;

namespace {

enum Kind { STEM, POOL, CONV1, CONV3 };
// buffers: two that the block outputs alternate between (conv1 and pool1 start the alternation), branch2a's
// output -- the only one a 3x3 reads, hence the only one whose halo has to be zero --, branch2b's, the projection
enum Buf { XA, XB, T1, T2, SC, NBUF };

struct ResOp {
  std::string name;
  Kind kind = CONV1;
  int Cin = 0, Cout = 0, k = 1, stride = 1, relu = 1;
  int lin = 0, lout = 0;          // geometry level of input / output (extent_at)
  int in = -1, out = -1, res = -1;
  bool zero_out = false;          // first branch2a of a stage: clear T1 (its geometry changes here)
  float* W = nullptr;             // [k][k][Cin][Cout] as set (folded)
  float* b = nullptr;             // [Cout]
  float* Bp = nullptr;            // PK pack (every convolution behind conv1)
  int Np = 0;
  bool w_set = false, b_set = false;
};

// level 0: the image; 1: conv1; 2: pool1 = res2; 3, 4, 5: res3, res4, res5
int extent_at(int n, int level) {
  if (level >= 1) n = resnet_half(n);
  if (level >= 2) n = resnet_pool_out(n);
  for (int l = 3; l <= level; ++l) n = resnet_half(n);
  return n;
}

struct Tmp {
  void* p = nullptr;
  ~Tmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  float* f() const { return static_cast<float*>(p); }
};

}  // namespace

struct n2nmn_resnet {
  int device = 0, max_N = 0, max_H = 0, max_W = 0, base = 64;
  std::vector<ResOp> ops;
  float* buf[NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t buf_floats[NBUF] = {0, 0, 0, 0, 0};
  void* image = nullptr;          // the last forward's input (get_layer and the replay run from it)
  float mean[3] = {123.68f, 116.779f, 103.939f};
  bool committed = false;
  int last_N = 0, last_H = 0, last_W = 0, last_u8 = 0;
  int valid_upto = -1;            // ops [0, valid_upto] of the last forward are what the buffers hold
};

namespace {

void resnet_free(n2nmn_resnet* r) {
  for (auto& o : r->ops) {
    if (o.W) (void)hipFree(o.W);
    if (o.b) (void)hipFree(o.b);
    if (o.Bp) (void)hipFree(o.Bp);
  }
  for (float* p : r->buf)
    if (p) (void)hipFree(p);
  if (r->image) (void)hipFree(r->image);
  delete r;
}

// "res4b7" is the block output, which branch2c's epilogue forms: an alias of "res4b7_branch2c"
int find_op(const n2nmn_resnet* r, std::string name) {
  if (name.compare(0, 3, "res") == 0 && name.find('_') == std::string::npos) name += "_branch2c";
  for (size_t i = 0; i < r->ops.size(); ++i)
    if (r->ops[i].name == name) return (int)i;
  return -1;
}

std::string block_name(int stage, int j, int count) {
  std::string s = "res" + std::to_string(stage + 2);
  if (count <= 3 || j == 0) return s + (char)('a' + j);
  return s + "b" + std::to_string(j);
}

void build_schedule(n2nmn_resnet* r, const int blocks[4]) {
  const int base = r->base;
  ResOp c1;
  c1.name = "conv1"; c1.kind = STEM; c1.Cin = 3; c1.Cout = base; c1.k = 7; c1.stride = 2;
  c1.lin = 0; c1.lout = 1; c1.out = XA;
  r->ops.push_back(c1);
  ResOp p1;
  p1.name = "pool1"; p1.kind = POOL; p1.Cin = p1.Cout = base; p1.k = 3; p1.stride = 2;
  p1.lin = 1; p1.lout = 2; p1.in = XA; p1.out = XB;
  r->ops.push_back(p1);
  int cur = XB, cin = base;
  for (int st = 0; st < 4; ++st) {
    const int width = base << st, cout = 4 * width;
    for (int j = 0; j < blocks[st]; ++j) {
      const std::string bn = block_name(st, j, blocks[st]);
      const int stride = (j == 0 && st > 0) ? 2 : 1;
      const int lin = (j == 0 && st > 0) ? st + 1 : st + 2, lout = st + 2;
      const int nxt = cur == XA ? XB : XA;
      if (j == 0) {
        ResOp o;
        o.name = bn + "_branch1"; o.Cin = cin; o.Cout = cout; o.stride = stride; o.relu = 0;
        o.lin = lin; o.lout = lout; o.in = cur; o.out = SC;
        r->ops.push_back(o);
      }
      ResOp a;
      a.name = bn + "_branch2a"; a.Cin = cin; a.Cout = width; a.stride = stride;
      a.lin = lin; a.lout = lout; a.in = cur; a.out = T1; a.zero_out = j == 0;
      r->ops.push_back(a);
      ResOp b;
      b.name = bn + "_branch2b"; b.kind = CONV3; b.Cin = width; b.Cout = width; b.k = 3;
      b.lin = lout; b.lout = lout; b.in = T1; b.out = T2;
      r->ops.push_back(b);
      ResOp c;
      c.name = bn + "_branch2c"; c.Cin = width; c.Cout = cout;
      c.lin = lout; c.lout = lout; c.in = T2; c.out = nxt; c.res = j == 0 ? SC : cur;
      r->ops.push_back(c);
      cur = nxt;
      cin = cout;
    }
  }
}

ResConv1Args conv1_args(const n2nmn_resnet* r, const ResOp& o, int N, int H, int W) {
  return ResConv1Args{r->buf[o.in], r->buf[o.out], o.res >= 0 ? r->buf[o.res] : nullptr, o.Bp, o.b, N,
                      extent_at(H, o.lin), extent_at(W, o.lin), extent_at(H, o.lout), extent_at(W, o.lout),
                      o.Cin, o.Cout, o.Np, o.stride, o.relu};
}

VggConvArgs conv3_args(const n2nmn_resnet* r, const ResOp& o, int N, int H, int W) {
  return VggConvArgs{r->buf[o.in], r->buf[o.out], o.Bp, o.b, N, extent_at(H, o.lout), extent_at(W, o.lout), o.Cin,
                     o.Cout, o.Np};
}

// can ops [0, n) run on N x H x W: the tiles' 32-bit offsets
int check_geometry(const n2nmn_resnet* r, int N, int H, int W, const char* what) {
  for (const auto& o : r->ops) {
    const bool ok = o.kind == CONV1 ? resnet_conv1x1_supported(conv1_args(r, o, N, H, W))
                  : o.kind == CONV3 ? vgg_conv3_supported(conv3_args(r, o, N, H, W))
                                    : vgg_halo_floats(N, extent_at(H, o.lin), extent_at(W, o.lin), o.Cout) < ((size_t)1 << 31);
    N2_REQUIRE(ok, N2NMN_ECAPACITY, std::string(what) + ": " + o.name + ": activation too large for the tile's 32-bit offsets");
  }
  return N2NMN_OK;
}

// ops [first, upto] of the schedule on the handle's saved image
int run_ops(n2nmn_resnet* r, int first, int upto, hipStream_t s) {
  const int N = r->last_N, H = r->last_H, W = r->last_W;
  for (int i = first; i <= upto; ++i) {
    const ResOp& o = r->ops[i];
    const int hi = extent_at(H, o.lin), wi = extent_at(W, o.lin);
    switch (o.kind) {
      case STEM:
        launch_resnet_stem(r->image, r->last_u8, N, hi, wi, o.W, o.b, r->mean, o.Cout, r->buf[o.out], s);
        break;
      case POOL:
        launch_resnet_pool(r->buf[o.in], N, hi, wi, o.Cin, r->buf[o.out], s);
        break;
      case CONV1:
        if (o.zero_out)
          N2_HIP(hipMemsetAsync(r->buf[o.out], 0,
                                sizeof(float) * vgg_halo_floats(N, extent_at(H, o.lout), extent_at(W, o.lout), o.Cout), s));
        launch_resnet_conv1x1(conv1_args(r, o, N, H, W), s);
        break;
      case CONV3:
        launch_vgg_conv3(conv3_args(r, o, N, H, W), s);
        break;
    }
  }
  return N2NMN_OK;
}

size_t weight_floats(const ResOp& o) { return (size_t)o.k * o.k * o.Cin * o.Cout; }

}  // namespace

extern "C" {

int n2nmn_resnet_create(int device, int max_N, int max_H, int max_W, const int blocks[4], int base_width,
                        n2nmn_resnet** out) {
  N2_REQUIRE(out && blocks, N2NMN_EINVAL, "resnet_create: null argument");
  *out = nullptr;
  N2_REQUIRE(max_N > 0 && max_H > 0 && max_W > 0, N2NMN_EINVAL, "resnet_create: max_N, max_H and max_W must be positive");
  for (int st = 0; st < 4; ++st)
    N2_REQUIRE(blocks[st] >= 1 && blocks[st] <= 64, N2NMN_EINVAL, "resnet_create: every stage needs 1 .. 64 blocks");
  N2_REQUIRE(base_width > 0 && base_width <= 256 && base_width % 32 == 0, N2NMN_EINVAL,
             "resnet_create: base_width must be a multiple of 32 (the k stage of the convolution tiles), at most 256");
  N2_HIP(hipSetDevice(device));
  n2nmn_resnet* r = new n2nmn_resnet;
  r->device = device; r->max_N = max_N; r->max_H = max_H; r->max_W = max_W; r->base = base_width;
  build_schedule(r, blocks);
  for (auto& o : r->ops) {
    if (o.kind == CONV1 || o.kind == CONV3) o.Np = round_up(o.Cout, 128);
    if (o.out >= 0)
      r->buf_floats[o.out] = std::max(r->buf_floats[o.out], vgg_halo_floats(max_N, extent_at(max_H, o.lout),
                                                                            extent_at(max_W, o.lout), o.Cout));
  }
  const int rc = check_geometry(r, max_N, max_H, max_W, "resnet_create");
  if (rc) {
    resnet_free(r);
    return rc;
  }
  hipError_t e = hipMalloc(&r->image, sizeof(float) * (size_t)max_N * max_H * max_W * 3);
  for (int b = 0; b < NBUF; ++b)
    if (e == hipSuccess) e = hipMalloc((void**)&r->buf[b], sizeof(float) * r->buf_floats[b]);
  for (auto& o : r->ops) {
    if (o.kind == POOL) continue;
    if (e == hipSuccess) e = hipMalloc((void**)&o.W, sizeof(float) * weight_floats(o));
    if (e == hipSuccess) e = hipMalloc((void**)&o.b, sizeof(float) * o.Cout);
    if (o.Np && e == hipSuccess) e = hipMalloc((void**)&o.Bp, sizeof(float) * o.k * o.k * o.Cin * o.Np);
  }
  if (e != hipSuccess) {
    set_last_error(std::string("resnet_create: hipMalloc: ") + hipGetErrorString(e));
    resnet_free(r);
    return N2NMN_EHIP;
  }
  *out = r;
  return N2NMN_OK;
}

int n2nmn_resnet_destroy(n2nmn_resnet* resnet) {
  if (!resnet) return N2NMN_OK;
  (void)hipSetDevice(resnet->device);
  (void)hipDeviceSynchronize();          // (destroy only: kernels may still read the buffers)
  resnet_free(resnet);
  return N2NMN_OK;
}

int n2nmn_resnet_set_mean(n2nmn_resnet* resnet, const float mean[3]) {
  N2_REQUIRE(resnet && mean, N2NMN_EINVAL, "resnet_set_mean: null argument");
  for (int c = 0; c < 3; ++c) resnet->mean[c] = mean[c];
  return N2NMN_OK;
}

int n2nmn_resnet_set_weight(n2nmn_resnet* resnet, const char* name, const float* data, const int64_t* shape,
                            int ndim) {
  N2_REQUIRE(resnet && name && data && shape, N2NMN_EINVAL, "resnet_set_weight: null argument");
  const std::string full(name);
  const size_t slash = full.find('/');
  const std::string lname = full.substr(0, slash), kind = slash == std::string::npos ? "" : full.substr(slash + 1);
  int i = -1;
  for (size_t j = 0; j < resnet->ops.size(); ++j)
    if (resnet->ops[j].name == lname) i = (int)j;
  if (i < 0 || resnet->ops[i].kind == POOL || (kind != "weights" && kind != "biases")) {
    set_last_error("resnet_set_weight: unknown variable '" + full + "' (expected conv1/weights ... " +
                   resnet->ops.back().name + "/biases)");
    return N2NMN_EKEY;
  }
  ResOp& o = resnet->ops[i];
  const bool isw = kind == "weights";
  const bool ok = isw ? (ndim == 4 && shape[0] == o.k && shape[1] == o.k && shape[2] == o.Cin && shape[3] == o.Cout)
                      : (ndim == 1 && shape[0] == o.Cout);
  if (!ok) {
    std::string got;
    for (int d = 0; d < ndim; ++d) got += (d ? ", " : "") + std::to_string((long long)shape[d]);
    const std::string ks = std::to_string(o.k);
    set_last_error("resnet_set_weight: " + full + " has shape [" + got + "], expected " +
                   (isw ? "[" + ks + ", " + ks + ", " + std::to_string(o.Cin) + ", " + std::to_string(o.Cout) + "]"
                        : "[" + std::to_string(o.Cout) + "]"));
    return N2NMN_EINVAL;
  }
  N2_HIP(hipSetDevice(resnet->device));
  const size_t bytes = sizeof(float) * (isw ? weight_floats(o) : (size_t)o.Cout);
  N2_HIP(hipMemcpy(isw ? o.W : o.b, data, bytes, hipMemcpyDeviceToDevice));
  (isw ? o.w_set : o.b_set) = true;
  resnet->committed = false;
  return N2NMN_OK;
}

int n2nmn_resnet_commit(n2nmn_resnet* resnet, n2nmn_stream stream) {
  N2_REQUIRE(resnet, N2NMN_EINVAL, "resnet_commit: null argument");
  for (const auto& o : resnet->ops)
    if (o.kind != POOL && !(o.w_set && o.b_set)) {
      set_last_error("resnet_commit: " + o.name + (o.w_set ? "/biases" : "/weights") + " was never set");
      return N2NMN_ENOWEIGHT;
    }
  N2_HIP(hipSetDevice(resnet->device));
  for (auto& o : resnet->ops)
    if (o.Bp) launch_pack_pk(o.W, o.Cout, o.k * o.k * o.Cin, o.Cout, o.Bp, o.k * o.k * o.Cin, o.Np, S(stream));
  resnet->committed = true;
  return check_launch("resnet_commit");
}

int n2nmn_resnet_forward(n2nmn_resnet* resnet, const void* images, int is_uint8, int N, int H, int W, float* out,
                         n2nmn_stream stream) {
  N2_REQUIRE(resnet && images && out, N2NMN_EINVAL, "resnet_forward: null argument");
  N2_REQUIRE(resnet->committed, N2NMN_ENOWEIGHT, "resnet_forward: weights not committed (n2nmn_resnet_commit)");
  N2_REQUIRE(N > 0 && H > 0 && W > 0, N2NMN_EINVAL, "resnet_forward: N, H and W must be positive");
  N2_REQUIRE(N <= resnet->max_N && H <= resnet->max_H && W <= resnet->max_W, N2NMN_ECAPACITY,
             "resnet_forward: N x H x W = " + std::to_string(N) + " x " + std::to_string(H) + " x " + std::to_string(W) +
                 " exceeds the handle's " + std::to_string(resnet->max_N) + " x " + std::to_string(resnet->max_H) +
                 " x " + std::to_string(resnet->max_W));
  N2_HIP(hipSetDevice(resnet->device));
  hipStream_t s = S(stream);
  const int rc0 = check_geometry(resnet, N, H, W, "resnet_forward");
  if (rc0) return rc0;
  resnet->last_N = 0;
  resnet->valid_upto = -1;
  N2_HIP(hipMemcpyAsync(resnet->image, images, (size_t)N * H * W * 3 * (is_uint8 ? 1 : sizeof(float)),
                        hipMemcpyDeviceToDevice, s));
  resnet->last_N = N; resnet->last_H = H; resnet->last_W = W; resnet->last_u8 = is_uint8 ? 1 : 0;
  const int last = (int)resnet->ops.size() - 1;
  const int rc = run_ops(resnet, 0, last, s);
  if (rc) {
    resnet->last_N = 0;
    return rc;
  }
  const ResOp& o = resnet->ops[last];
  launch_vgg_unpad(resnet->buf[o.out], N, extent_at(H, o.lout), extent_at(W, o.lout), o.Cout, out, s);
  resnet->valid_upto = last;
  return check_launch("resnet_forward");
}

int n2nmn_resnet_get_layer(n2nmn_resnet* resnet, const char* layer, float* out, int64_t capacity, int64_t shape[4],
                           n2nmn_stream stream) {
  N2_REQUIRE(resnet && layer && shape, N2NMN_EINVAL, "resnet_get_layer: null argument");
  const int i = find_op(resnet, layer);
  if (i < 0) {
    set_last_error(std::string("resnet_get_layer: unknown layer '") + layer + "' (conv1, pool1, res2a_branch1 ... " +
                   resnet->ops.back().name + ")");
    return N2NMN_EKEY;
  }
  N2_REQUIRE(resnet->last_N > 0, N2NMN_EINVAL, "resnet_get_layer: no forward pass has run on this handle");
  const ResOp& o = resnet->ops[i];
  const int h = extent_at(resnet->last_H, o.lout), w = extent_at(resnet->last_W, o.lout);
  shape[0] = resnet->last_N; shape[1] = h; shape[2] = w; shape[3] = o.Cout;
  if (!out) return N2NMN_OK;               // shape query
  N2_REQUIRE(capacity >= shape[0] * shape[1] * shape[2] * shape[3], N2NMN_ECAPACITY,
             "resnet_get_layer: `out` holds fewer floats than the layer");
  N2_HIP(hipSetDevice(resnet->device));
  hipStream_t s = S(stream);
  if (resnet->valid_upto != i) {           // the buffers are shared: run the saved image up to this layer again
    resnet->valid_upto = -1;
    const int rc = run_ops(resnet, 0, i, s);
    if (rc) return rc;
    resnet->valid_upto = i;
  }
  launch_vgg_unpad(resnet->buf[o.out], resnet->last_N, h, w, o.Cout, out, s);
  return check_launch("resnet_get_layer");
}

int n2nmn_resnet_debug_replay(n2nmn_resnet* resnet, const char* layer, int iters, double* us_avg,
                              n2nmn_stream stream) {
  N2_REQUIRE(resnet && us_avg && iters > 0, N2NMN_EINVAL, "resnet_debug_replay: bad argument");
  int first = 0, upto = (int)resnet->ops.size() - 1;
  if (layer && *layer) {
    first = upto = find_op(resnet, layer);
    if (first < 0) {
      set_last_error(std::string("resnet_debug_replay: unknown layer '") + layer + "'");
      return N2NMN_EKEY;
    }
  }
  N2_REQUIRE(resnet->last_N > 0, N2NMN_EINVAL, "resnet_debug_replay: no forward pass has run on this handle");
  N2_HIP(hipSetDevice(resnet->device));
  hipStream_t s = S(stream);
  resnet->valid_upto = -1;                 // a single layer re-run reads whatever its input buffer holds by now
  hipEvent_t e0, e1;
  N2_HIP(hipEventCreate(&e0));
  N2_HIP(hipEventCreate(&e1));
  int rc = N2NMN_OK;
  for (int k = 0; k < 3 && !rc; ++k) rc = run_ops(resnet, first, upto, s);
  (void)hipEventRecord(e0, s);
  for (int k = 0; k < iters && !rc; ++k) rc = run_ops(resnet, first, upto, s);
  (void)hipEventRecord(e1, s);
  const hipError_t done = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) return rc;
  N2_HIP(done);
  if (first == 0) resnet->valid_upto = upto;
  *us_avg = 1e3 * ms / iters;
  return check_launch("resnet_debug_replay");
}

int n2nmn_resnet_debug_stem(const void* images, int is_uint8, const float* w, const float* bias, const float mean[3],
                            float* out, int N, int H, int W, int Cout, n2nmn_stream stream) {
  N2_REQUIRE(images && w && bias && mean && out, N2NMN_EINVAL, "resnet_debug_stem: null argument");
  N2_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0, N2NMN_EINVAL, "resnet_debug_stem: needs Cout % 4 == 0");
  const int ho = resnet_half(H), wo = resnet_half(W);
  Tmp hout;
  N2_HIP(hout.alloc(sizeof(float) * vgg_halo_floats(N, ho, wo, Cout)));
  hipStream_t s = S(stream);
  launch_resnet_stem(images, is_uint8, N, H, W, w, bias, mean, Cout, hout.f(), s);
  launch_vgg_unpad(hout.f(), N, ho, wo, Cout, out, s);
  N2_HIP(hipStreamSynchronize(s));          // debug entry only: the temporary is freed right away
  return check_launch("resnet_debug_stem");
}

int n2nmn_resnet_debug_pool(const float* in, float* out, int N, int H, int W, int C, n2nmn_stream stream) {
  N2_REQUIRE(in && out, N2NMN_EINVAL, "resnet_debug_pool: null argument");
  N2_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, N2NMN_EINVAL, "resnet_debug_pool: needs C % 4 == 0");
  const int ho = resnet_pool_out(H), wo = resnet_pool_out(W);
  Tmp hin, hout;
  const size_t in_b = sizeof(float) * vgg_halo_floats(N, H, W, C);
  N2_HIP(hin.alloc(in_b));
  N2_HIP(hout.alloc(sizeof(float) * vgg_halo_floats(N, ho, wo, C)));
  hipStream_t s = S(stream);
  N2_HIP(hipMemsetAsync(hin.p, 0, in_b, s));
  launch_vgg_pad(in, N, H, W, C, hin.f(), s);
  launch_resnet_pool(hin.f(), N, H, W, C, hout.f(), s);
  launch_vgg_unpad(hout.f(), N, ho, wo, C, out, s);
  N2_HIP(hipStreamSynchronize(s));          // debug entry only: the temporaries are freed right away
  return check_launch("resnet_debug_pool");
}

int n2nmn_resnet_debug_conv1x1(const float* in, const float* w, const float* bias, const float* residual, float* out,
                               int N, int H, int W, int Cin, int Cout, int stride, int relu, n2nmn_stream stream) {
  N2_REQUIRE(in && w && bias && out, N2NMN_EINVAL, "resnet_debug_conv1x1: null argument");
  N2_REQUIRE(stride == 1 || stride == 2, N2NMN_EINVAL, "resnet_debug_conv1x1: stride must be 1 or 2");
  N2_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, N2NMN_EINVAL, "resnet_debug_conv1x1: extents must be positive");
  const int ho = stride == 2 ? resnet_half(H) : H, wo = stride == 2 ? resnet_half(W) : W;
  const int Np = round_up(Cout, 128);
  ResConv1Args a{nullptr, nullptr, nullptr, nullptr, bias, N, H, W, ho, wo, Cin, Cout, Np, stride, relu};
  N2_REQUIRE(resnet_conv1x1_supported(a) && Cin % 4 == 0 && Cout % 4 == 0, N2NMN_EINVAL,
             "resnet_debug_conv1x1: needs Cin % 32 == 0, Cout % 4 == 0 and buffers below 4 GiB");
  Tmp hin, hout, hres, pack;
  const size_t in_b = sizeof(float) * vgg_halo_floats(N, H, W, Cin), out_b = sizeof(float) * vgg_halo_floats(N, ho, wo, Cout);
  N2_HIP(hin.alloc(in_b));
  N2_HIP(hout.alloc(out_b));
  N2_HIP(pack.alloc(sizeof(float) * Cin * Np));
  hipStream_t s = S(stream);
  N2_HIP(hipMemsetAsync(hin.p, 0, in_b, s));
  launch_vgg_pad(in, N, H, W, Cin, hin.f(), s);
  if (residual) {
    N2_HIP(hres.alloc(out_b));
    N2_HIP(hipMemsetAsync(hres.p, 0, out_b, s));
    launch_vgg_pad(residual, N, ho, wo, Cout, hres.f(), s);
  }
  launch_pack_pk(w, Cout, Cin, Cout, pack.f(), Cin, Np, s);
  a.in = hin.f(); a.out = hout.f(); a.res = hres.f(); a.Bp = pack.f();
  launch_resnet_conv1x1(a, s);
  launch_vgg_unpad(hout.f(), N, ho, wo, Cout, out, s);
  N2_HIP(hipStreamSynchronize(s));          // debug entry only: the temporaries are freed right away
  return check_launch("resnet_debug_conv1x1");
}

}  // extern "C"
