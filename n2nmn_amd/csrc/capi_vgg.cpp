// C ABI of the VGG-16 pool5 feature extractor (include/n2nmn.h section 9): the n2nmn_vgg handle, its weight
// store and the layer schedule of models_clevr/vgg_net.py:16-56.  Host code only; kernels: kernels_vgg.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/n2nmn.h"
#include "kernels.h"
#include "vgg_kernels.h"

#include "ctx.h"

using namespace n2nmn;

namespace {

struct VggLayer {
  std::string name;
  bool pool = false;
  int Cin = 0, Cout = 0;          // pool: Cin == Cout
  int level = 0;                  // the layer's INPUT extent is the image's halved (ceil) `level` times
  float* W = nullptr;             // [3][3][Cin][Cout] as set
  float* b = nullptr;             // [Cout]
  float* Bp = nullptr;            // PK pack [9 Cin / 4][Np][4] (conv layers behind conv1_1)
  int Np = 0;
  float* act = nullptr;           // haloed output at the handle's maximum geometry (pool5: none, it goes to `out`)
  size_t act_bytes = 0;
  bool w_set = false, b_set = false;
};

int half_n(int x, int times) {
  for (int i = 0; i < times; ++i) x = (x + 1) / 2;
  return x;
}

}  // namespace

struct n2nmn_vgg {
  int device = 0, max_N = 0, max_H = 0, max_W = 0;
  std::vector<VggLayer> layers;
  bool committed = false;
  int zero_H = 0, zero_W = 0;     // the image extent the halos are zero for (0: none yet)
  int last_N = 0, last_H = 0, last_W = 0;
};

namespace {

void vgg_free(n2nmn_vgg* v) {
  for (auto& l : v->layers) {
    if (l.W) (void)hipFree(l.W);
    if (l.b) (void)hipFree(l.b);
    if (l.Bp) (void)hipFree(l.Bp);
    if (l.act) (void)hipFree(l.act);
  }
  delete v;
}

int find_layer(const n2nmn_vgg* v, const std::string& name) {
  for (size_t i = 0; i < v->layers.size(); ++i)
    if (v->layers[i].name == name) return (int)i;
  return -1;
}

// Halos are zero for one image extent at a time: kernels write interiors only, so they stay zero from call to
// call (for any N: an image's pixels do not move with N).  When the extent changes, the buffers are cleared on
// the stream of the call that changes it.
int zero_halos(n2nmn_vgg* v, int H, int W, hipStream_t s) {
  if (v->zero_H == H && v->zero_W == W) return N2NMN_OK;
  v->zero_H = v->zero_W = 0;
  for (auto& l : v->layers)
    if (l.act) N2_HIP(hipMemsetAsync(l.act, 0, l.act_bytes, s));
  v->zero_H = H;
  v->zero_W = W;
  return N2NMN_OK;
}

// layers [0, upto] of the schedule on images of N x H x W; pool5 writes `out` (dense)
int run_layers(n2nmn_vgg* v, const void* images, int is_uint8, int N, int H, int W, int first, int upto, float* out,
               hipStream_t s) {
  for (int i = first; i <= upto; ++i) {
    VggLayer& l = v->layers[i];
    const int h = half_n(H, l.level), w = half_n(W, l.level);
    const float* in = i ? v->layers[i - 1].act : nullptr;
    if (i == 0) {
      launch_vgg_conv1(images, is_uint8, N, h, w, l.W, l.b, l.act, s);
    } else if (l.pool) {
      launch_vgg_pool(in, N, h, w, l.Cin, l.act ? l.act : out, l.act ? 1 : 0, s);
    } else {
      VggConvArgs a{in, l.act, l.Bp, l.b, N, h, w, l.Cin, l.Cout, l.Np};
      N2_REQUIRE(vgg_conv3_supported(a), N2NMN_ECAPACITY, "vgg_forward: " + l.name + ": activation too large for the tile's 32-bit offsets");
      launch_vgg_conv3(a, s);
    }
  }
  return N2NMN_OK;
}

struct Tmp {
  void* p = nullptr;
  ~Tmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  float* f() const { return static_cast<float*>(p); }
};

}  // namespace

extern "C" {

int n2nmn_vgg_create(int device, int max_N, int max_H, int max_W, n2nmn_vgg** out) {
  N2_REQUIRE(out, N2NMN_EINVAL, "vgg_create: null argument");
  *out = nullptr;
  N2_REQUIRE(max_N > 0 && max_H > 0 && max_W > 0, N2NMN_EINVAL, "vgg_create: max_N, max_H and max_W must be positive");
  N2_REQUIRE(vgg_halo_floats(max_N, max_H, max_W, 64) * 4 < ((size_t)1 << 32), N2NMN_ECAPACITY,
             "vgg_create: max_N * (max_H + 2) * (max_W + 2) * 64 floats must stay below 4 GiB (32-bit tile offsets)");
  N2_HIP(hipSetDevice(device));
  n2nmn_vgg* v = new n2nmn_vgg;
  v->device = device; v->max_N = max_N; v->max_H = max_H; v->max_W = max_W;
  static const int nconv[5] = {2, 2, 3, 3, 3}, width[5] = {64, 128, 256, 512, 512};
  int cin = 3;
  for (int g = 0; g < 5; ++g) {
    for (int j = 0; j < nconv[g]; ++j) {
      VggLayer l;
      l.name = "conv" + std::to_string(g + 1) + "_" + std::to_string(j + 1);
      l.Cin = cin; l.Cout = width[g]; l.level = g;
      cin = width[g];
      v->layers.push_back(l);
    }
    VggLayer p;
    p.name = "pool" + std::to_string(g + 1);
    p.pool = true; p.Cin = p.Cout = cin; p.level = g;
    v->layers.push_back(p);
  }
  hipError_t e = hipSuccess;
  for (auto& l : v->layers) {
    if (!l.pool) {
      if (e == hipSuccess) e = hipMalloc((void**)&l.W, sizeof(float) * 9 * l.Cin * l.Cout);
      if (e == hipSuccess) e = hipMalloc((void**)&l.b, sizeof(float) * l.Cout);
      if (l.Cin != 3) {
        l.Np = round_up(l.Cout, 128);
        if (e == hipSuccess) e = hipMalloc((void**)&l.Bp, sizeof(float) * 9 * l.Cin * l.Np);
      }
    }
    if (l.name != "pool5") {
      const int lv = l.level + (l.pool ? 1 : 0);
      l.act_bytes = sizeof(float) * vgg_halo_floats(max_N, half_n(max_H, lv), half_n(max_W, lv), l.Cout);
      if (e == hipSuccess) e = hipMalloc((void**)&l.act, l.act_bytes);
    }
  }
  if (e != hipSuccess) {
    set_last_error(std::string("vgg_create: hipMalloc: ") + hipGetErrorString(e));
    vgg_free(v);
    return N2NMN_EHIP;
  }
  *out = v;
  return N2NMN_OK;
}

int n2nmn_vgg_destroy(n2nmn_vgg* vgg) {
  if (!vgg) return N2NMN_OK;
  (void)hipSetDevice(vgg->device);
  (void)hipDeviceSynchronize();          // (destroy only: kernels may still read the buffers)
  vgg_free(vgg);
  return N2NMN_OK;
}

int n2nmn_vgg_set_weight(n2nmn_vgg* vgg, const char* name, const float* data, const int64_t* shape, int ndim) {
  N2_REQUIRE(vgg && name && data && shape, N2NMN_EINVAL, "vgg_set_weight: null argument");
  const std::string full(name);
  const size_t slash = full.find('/');
  const std::string lname = full.substr(0, slash), kind = slash == std::string::npos ? "" : full.substr(slash + 1);
  const int i = find_layer(vgg, lname);
  if (i < 0 || vgg->layers[i].pool || (kind != "weights" && kind != "biases")) {
    set_last_error("vgg_set_weight: unknown variable '" + full + "' (expected conv1_1/weights ... conv5_3/biases)");
    return N2NMN_EKEY;
  }
  VggLayer& l = vgg->layers[i];
  const bool isw = kind == "weights";
  const bool ok = isw ? (ndim == 4 && shape[0] == 3 && shape[1] == 3 && shape[2] == l.Cin && shape[3] == l.Cout)
                      : (ndim == 1 && shape[0] == l.Cout);
  if (!ok) {
    std::string got;
    for (int d = 0; d < ndim; ++d) got += (d ? ", " : "") + std::to_string((long long)shape[d]);
    set_last_error("vgg_set_weight: " + full + " has shape [" + got + "], expected " +
                   (isw ? "[3, 3, " + std::to_string(l.Cin) + ", " + std::to_string(l.Cout) + "]"
                        : "[" + std::to_string(l.Cout) + "]"));
    return N2NMN_EINVAL;
  }
  N2_HIP(hipSetDevice(vgg->device));
  const size_t bytes = sizeof(float) * (isw ? (size_t)9 * l.Cin * l.Cout : (size_t)l.Cout);
  N2_HIP(hipMemcpy(isw ? l.W : l.b, data, bytes, hipMemcpyDeviceToDevice));
  (isw ? l.w_set : l.b_set) = true;
  vgg->committed = false;
  return N2NMN_OK;
}

int n2nmn_vgg_commit(n2nmn_vgg* vgg, n2nmn_stream stream) {
  N2_REQUIRE(vgg, N2NMN_EINVAL, "vgg_commit: null argument");
  for (const auto& l : vgg->layers)
    if (!l.pool && !(l.w_set && l.b_set)) {
      set_last_error("vgg_commit: " + l.name + (l.w_set ? "/biases" : "/weights") + " was never set");
      return N2NMN_ENOWEIGHT;
    }
  N2_HIP(hipSetDevice(vgg->device));
  for (auto& l : vgg->layers)
    if (l.Bp) launch_pack_pk(l.W, l.Cout, 9 * l.Cin, l.Cout, l.Bp, 9 * l.Cin, l.Np, S(stream));
  vgg->committed = true;
  return check_launch("vgg_commit");
}

int n2nmn_vgg_forward(n2nmn_vgg* vgg, const void* images, int is_uint8, int N, int H, int W, float* out,
                      n2nmn_stream stream) {
  N2_REQUIRE(vgg && images && out, N2NMN_EINVAL, "vgg_forward: null argument");
  N2_REQUIRE(vgg->committed, N2NMN_ENOWEIGHT, "vgg_forward: weights not committed (n2nmn_vgg_commit)");
  N2_REQUIRE(N > 0 && H > 0 && W > 0, N2NMN_EINVAL, "vgg_forward: N, H and W must be positive");
  N2_REQUIRE(N <= vgg->max_N && H <= vgg->max_H && W <= vgg->max_W, N2NMN_ECAPACITY,
             "vgg_forward: N x H x W = " + std::to_string(N) + " x " + std::to_string(H) + " x " + std::to_string(W) +
                 " exceeds the handle's " + std::to_string(vgg->max_N) + " x " + std::to_string(vgg->max_H) + " x " +
                 std::to_string(vgg->max_W));
  N2_HIP(hipSetDevice(vgg->device));
  hipStream_t s = S(stream);
  const int rc0 = zero_halos(vgg, H, W, s);
  if (rc0) return rc0;
  vgg->last_N = 0;
  const int rc = run_layers(vgg, images, is_uint8, N, H, W, 0, (int)vgg->layers.size() - 1, out, s);
  if (rc) return rc;
  vgg->last_N = N; vgg->last_H = H; vgg->last_W = W;
  return check_launch("vgg_forward");
}

int n2nmn_vgg_get_layer(n2nmn_vgg* vgg, const char* layer, float* out, int64_t capacity, int64_t shape[4],
                        n2nmn_stream stream) {
  N2_REQUIRE(vgg && layer && shape, N2NMN_EINVAL, "vgg_get_layer: null argument");
  const int i = find_layer(vgg, layer);
  if (i < 0) {
    set_last_error(std::string("vgg_get_layer: unknown layer '") + layer + "' (conv1_1 ... conv5_3, pool1 ... pool5)");
    return N2NMN_EKEY;
  }
  N2_REQUIRE(vgg->last_N > 0, N2NMN_EINVAL, "vgg_get_layer: no forward pass has run on this handle");
  const VggLayer& l = vgg->layers[i];
  const int lv = l.level + (l.pool ? 1 : 0);
  const int h = half_n(vgg->last_H, lv), w = half_n(vgg->last_W, lv);
  shape[0] = vgg->last_N; shape[1] = h; shape[2] = w; shape[3] = l.Cout;
  if (!out) return N2NMN_OK;               // shape query
  N2_REQUIRE(capacity >= shape[0] * shape[1] * shape[2] * shape[3], N2NMN_ECAPACITY,
             "vgg_get_layer: `out` holds fewer floats than the layer");
  N2_HIP(hipSetDevice(vgg->device));
  if (l.act) launch_vgg_unpad(l.act, vgg->last_N, h, w, l.Cout, out, S(stream));
  else launch_vgg_pool(vgg->layers[i - 1].act, vgg->last_N, half_n(vgg->last_H, l.level), half_n(vgg->last_W, l.level),
                       l.Cin, out, 0, S(stream));
  return check_launch("vgg_get_layer");
}

int n2nmn_vgg_debug_replay(n2nmn_vgg* vgg, const char* layer, int iters, double* us_avg, n2nmn_stream stream) {
  N2_REQUIRE(vgg && layer && us_avg && iters > 0, N2NMN_EINVAL, "vgg_debug_replay: bad argument");
  const int i = find_layer(vgg, layer);
  if (i <= 0) {
    set_last_error(std::string("vgg_debug_replay: unknown or unsupported layer '") + layer + "' (conv1_2 ... pool5)");
    return N2NMN_EKEY;
  }
  N2_REQUIRE(vgg->last_N > 0, N2NMN_EINVAL, "vgg_debug_replay: no forward pass has run on this handle");
  N2_HIP(hipSetDevice(vgg->device));
  hipStream_t s = S(stream);
  Tmp sink;                                  // pool5 writes the caller's buffer in a forward; here a scratch one
  if (!vgg->layers[i].act)
    N2_HIP(sink.alloc(sizeof(float) * (size_t)vgg->last_N * half_n(vgg->last_H, 5) * half_n(vgg->last_W, 5) * 512));
  hipEvent_t e0, e1;
  N2_HIP(hipEventCreate(&e0));
  N2_HIP(hipEventCreate(&e1));
  int rc = N2NMN_OK;
  for (int k = 0; k < 3 && !rc; ++k) rc = run_layers(vgg, nullptr, 0, vgg->last_N, vgg->last_H, vgg->last_W, i, i, sink.f(), s);
  (void)hipEventRecord(e0, s);
  for (int k = 0; k < iters && !rc; ++k) rc = run_layers(vgg, nullptr, 0, vgg->last_N, vgg->last_H, vgg->last_W, i, i, sink.f(), s);
  (void)hipEventRecord(e1, s);
  const hipError_t done = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) return rc;
  N2_HIP(done);
  *us_avg = 1e3 * ms / iters;
  return check_launch("vgg_debug_replay");
}

int n2nmn_vgg_debug_conv(const float* in, const float* W, const float* bias, float* out, int N, int H, int Wd, int Cin,
                         int Cout, n2nmn_stream stream) {
  N2_REQUIRE(in && W && bias && out, N2NMN_EINVAL, "vgg_debug_conv: null argument");
  const int Np = round_up(Cout, 128);
  Tmp hin, hout, pack;
  VggConvArgs a{nullptr, nullptr, nullptr, bias, N, H, Wd, Cin, Cout, Np};
  N2_REQUIRE(vgg_conv3_supported(a) && Cout % 4 == 0, N2NMN_EINVAL,
             "vgg_debug_conv: needs Cin % 32 == 0, Cout % 4 == 0 and buffers below 4 GiB");
  const size_t in_b = sizeof(float) * vgg_halo_floats(N, H, Wd, Cin), out_b = sizeof(float) * vgg_halo_floats(N, H, Wd, Cout);
  N2_HIP(hin.alloc(in_b));
  N2_HIP(hout.alloc(out_b));
  N2_HIP(pack.alloc(sizeof(float) * 9 * Cin * Np));
  hipStream_t s = S(stream);
  N2_HIP(hipMemsetAsync(hin.p, 0, in_b, s));
  N2_HIP(hipMemsetAsync(hout.p, 0, out_b, s));
  launch_vgg_pad(in, N, H, Wd, Cin, hin.f(), s);
  launch_pack_pk(W, Cout, 9 * Cin, Cout, pack.f(), 9 * Cin, Np, s);
  a.in = hin.f(); a.out = hout.f(); a.Bp = pack.f();
  launch_vgg_conv3(a, s);
  launch_vgg_unpad(hout.f(), N, H, Wd, Cout, out, s);
  N2_HIP(hipStreamSynchronize(s));          // debug entry only: the temporaries are freed right away
  return check_launch("vgg_debug_conv");
}

int n2nmn_vgg_debug_pool(const float* in, float* out, int N, int H, int W, int C, n2nmn_stream stream) {
  N2_REQUIRE(in && out, N2NMN_EINVAL, "vgg_debug_pool: null argument");
  N2_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, N2NMN_EINVAL, "vgg_debug_pool: needs C % 4 == 0");
  Tmp hin;
  const size_t in_b = sizeof(float) * vgg_halo_floats(N, H, W, C);
  N2_HIP(hin.alloc(in_b));
  hipStream_t s = S(stream);
  N2_HIP(hipMemsetAsync(hin.p, 0, in_b, s));
  launch_vgg_pad(in, N, H, W, C, hin.f(), s);
  launch_vgg_pool(hin.f(), N, H, W, C, out, 0, s);
  N2_HIP(hipStreamSynchronize(s));          // debug entry only: the temporary is freed right away
  return check_launch("vgg_debug_pool");
}

}  // extern "C"
