// Fused AdamW for mixed precision: bf16/fp16/fp32 params, fp32 master +
// moments + grads. One HBM sweep per tensor: grad scale (dp-average
// remainder x clip coefficient x inv loss scale), decoupled weight decay,
// moment updates, bias-corrected step, master update, low-precision
// write-back.
//
// Replaces the DeepSpeed fused-Adam + fp16-wrapper path the reference
// configures (conf/...yaml:122-128,137-143).
// Oracle: MixedPrecisionAdamW's torch._foreach eager path (tests share it).
#include "common.h"

namespace lpp {

template <typename T, int VEC>
__global__ void adamw_kernel(T* __restrict__ p, float* __restrict__ master,
                             const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float wd, float bias1, float bias2,
                             float grad_scale) {
  using PT = Pack<T, VEC>;
  using PF = Pack<float, VEC>;
  const float step_size = lr / bias1;
  const float inv_sqrt_bias2 = rsqrtf(bias2);
  const float decay = 1.f - lr * wd;
  const int64_t n_vec = n / VEC;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_vec;
       i += (int64_t)gridDim.x * blockDim.x) {
    PF gp = reinterpret_cast<const PF*>(g)[i];
    PF mp = reinterpret_cast<PF*>(m)[i];
    PF vp = reinterpret_cast<PF*>(v)[i];
    PF w = reinterpret_cast<PF*>(master)[i];
    PT out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float gk = gp.v[k] * grad_scale;
      float mk = beta1 * mp.v[k] + (1.f - beta1) * gk;
      float vk = beta2 * vp.v[k] + (1.f - beta2) * gk * gk;
      float wk = w.v[k] * decay;
      wk -= step_size * mk / (sqrtf(vk) * inv_sqrt_bias2 + eps);
      mp.v[k] = mk;
      vp.v[k] = vk;
      w.v[k] = wk;
      out.v[k] = from_f32<T>(wk);
    }
    reinterpret_cast<PF*>(m)[i] = mp;
    reinterpret_cast<PF*>(v)[i] = vp;
    reinterpret_cast<PF*>(master)[i] = w;
    reinterpret_cast<PT*>(p)[i] = out;
  }
  // scalar tail
  const int64_t tail = n_vec * VEC;
  for (int64_t i = tail + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gk = g[i] * grad_scale;
    float mk = beta1 * m[i] + (1.f - beta1) * gk;
    float vk = beta2 * v[i] + (1.f - beta2) * gk * gk;
    float wk = master[i] * decay;
    wk -= step_size * mk / (sqrtf(vk) * inv_sqrt_bias2 + eps);
    m[i] = mk;
    v[i] = vk;
    master[i] = wk;
    p[i] = from_f32<T>(wk);
  }
}

// adamw_kernel's scalar tail over the whole tensor, for a tensor whose
// parameter, master, grad or moments do not start on a packet boundary.
template <typename T>
__global__ LPP_NO_PACKED_F32 void adamw_kernel_s(
    T* __restrict__ p, float* __restrict__ master, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v, int64_t n, float lr, float beta1, float beta2,
    float eps, float wd, float bias1, float bias2, float grad_scale) {
  const float step_size = lr / bias1;
  const float inv_sqrt_bias2 = rsqrtf(bias2);
  const float decay = 1.f - lr * wd;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gk = g[i] * grad_scale;
    float mk = beta1 * m[i] + (1.f - beta1) * gk;
    float vk = beta2 * v[i] + (1.f - beta2) * gk * gk;
    float wk = master[i] * decay;
    wk -= step_size * mk / (sqrtf(vk) * inv_sqrt_bias2 + eps);
    m[i] = mk;
    v[i] = vk;
    master[i] = wk;
    p[i] = from_f32<T>(wk);
  }
}

}  // namespace lpp

void fused_adamw(std::vector<at::Tensor> params, std::vector<at::Tensor> masters,
                 std::vector<at::Tensor> grads, std::vector<at::Tensor> exp_avg,
                 std::vector<at::Tensor> exp_avg_sq, double lr, double beta1, double beta2,
                 double eps, double weight_decay, double bias1, double bias2,
                 double grad_scale) {
  auto stream = lpp::current_stream();
  TORCH_CHECK(masters.size() == params.size() && grads.size() == params.size() &&
                  exp_avg.size() == params.size() && exp_avg_sq.size() == params.size(),
              "fused_adamw: list lengths differ");
  for (size_t t = 0; t < params.size(); ++t) {
    auto& p = params[t];
    const int64_t n = p.numel();
    TORCH_CHECK(p.is_cuda() && p.is_contiguous());
    for (const at::Tensor* s : {&masters[t], &grads[t], &exp_avg[t], &exp_avg_sq[t]})
      TORCH_CHECK(s->is_cuda() && s->is_contiguous() && s->scalar_type() == at::kFloat &&
                      s->numel() == n,
                  "fused_adamw: master/grad/moments must be contiguous fp32 of the param's size");
    LPP_DISPATCH_FLOAT(p.scalar_type(), "fused_adamw", [&] {
      constexpr int VEC = 4;  // 4 fp32 state elems = 16B; param pack 4*sizeof(T)
      const int grid = lpp::grid_for((n + VEC - 1) / VEC, 256);
      float* mp = masters[t].data_ptr<float>();
      float* gp = grads[t].data_ptr<float>();
      float* m1 = exp_avg[t].data_ptr<float>();
      float* m2 = exp_avg_sq[t].data_ptr<float>();
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, (scalar_t*)p.data_ptr(), mp,
                           gp, m1, m2, n, (float)lr, (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay, (float)bias1, (float)bias2, (float)grad_scale);
      };
      // Per tensor: a grad view behind a tensor of numel % 4 != 0, or a ZeRO-1
      // shard cut at an odd element, is not packet-aligned.
      if (lpp::aligned(p.data_ptr(), VEC * sizeof(scalar_t)) && lpp::aligned(mp, 16) &&
          lpp::aligned(gp, 16) && lpp::aligned(m1, 16) && lpp::aligned(m2, 16))
        launch(lpp::adamw_kernel<scalar_t, VEC>);
      else
        launch(lpp::adamw_kernel_s<scalar_t>);
    });
  }
  LPP_CHECK_HIP(hipGetLastError());
}
