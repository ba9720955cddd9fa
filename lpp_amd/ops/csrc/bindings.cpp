// Python bindings for the lpp_amd gfx950 kernel extension.
#include <torch/extension.h>

#include <string>
#include <tuple>
#include <vector>

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor weight, double eps);
std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor weight,
                                    at::Tensor invrms);
std::vector<at::Tensor> rmsnorm_bwd_fused(std::vector<at::Tensor> dys, at::Tensor x,
                                          at::Tensor weight, at::Tensor invrms,
                                          c10::optional<at::Tensor> dres, bool want_t);
at::Tensor rope_fwd(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, int64_t pos_offset);
at::Tensor rope_bwd(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t, int64_t pos_offset);
std::vector<at::Tensor> rope_bwd_t(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t,
                                   int64_t pos_offset);
at::Tensor swiglu_fwd(at::Tensor gate, at::Tensor up);
std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor gate, at::Tensor up);
std::vector<at::Tensor> swiglu_bwd_t(at::Tensor dy, at::Tensor gate, at::Tensor up);
std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits, at::Tensor labels);
at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor labels, at::Tensor lse,
                             double scale);
std::vector<at::Tensor> attention_fwd(at::Tensor q, at::Tensor k, at::Tensor v);
std::vector<at::Tensor> attention_bwd(at::Tensor dO, at::Tensor q, at::Tensor k,
                                      at::Tensor v, at::Tensor o, at::Tensor lse2);
std::vector<at::Tensor> attention_fwd_docs(at::Tensor q, at::Tensor k, at::Tensor v,
                                           at::Tensor doc_start);
std::vector<at::Tensor> attention_bwd_docs(at::Tensor dO, at::Tensor q, at::Tensor k,
                                           at::Tensor v, at::Tensor o, at::Tensor lse2,
                                           at::Tensor doc_start, at::Tensor doc_end);
void attention_set_block_order(int64_t mode);
int64_t attention_get_block_order();
at::Tensor attention_block_order(int64_t kind, int64_t nblk, int64_t nheads, int64_t G,
                                 int64_t mode);
at::Tensor attention_lds_addresses(std::string pattern, int64_t shape, int64_t idx);
std::vector<double> attention_time_kernel(std::string kernel, at::Tensor dO, at::Tensor q,
                                          at::Tensor k, at::Tensor v, at::Tensor o,
                                          at::Tensor lse2, int64_t mode, int64_t G,
                                          int64_t warmup, int64_t reps,
                                          c10::optional<at::Tensor> doc_start,
                                          c10::optional<at::Tensor> doc_end);
at::Tensor attention_decode(at::Tensor q, at::Tensor k_new, at::Tensor v_new,
                            at::Tensor k_cache, at::Tensor v_cache, at::Tensor cos_t,
                            at::Tensor sin_t, c10::optional<at::Tensor> positions,
                            c10::optional<at::Tensor> rows,
                            c10::optional<at::Tensor> lengths, int64_t uniform_pos,
                            int64_t max_len, int64_t chunk);
int64_t attention_decode_chunk();
at::Tensor mfma_test_16x16x32(at::Tensor A, at::Tensor B);
void wgrad_f32_accum(at::Tensor x, at::Tensor dy, at::Tensor dw);
void wgrad_f32_accum_pre(at::Tensor xT, at::Tensor dyT, at::Tensor dw);
void wgrad_bf16d_pre(at::Tensor xT, at::Tensor dyT, at::Tensor out);
at::Tensor transpose2d(at::Tensor in);
void accum_bf16_f32(at::Tensor dst, at::Tensor src);
std::vector<std::tuple<int64_t, double, std::string>> wgrad_tune(int64_t T, int64_t in,
                                                                 int64_t out,
                                                                 int64_t reps,
                                                                 int64_t kind);
void wgrad_set_algo(int64_t T, int64_t in, int64_t out, int64_t index, int64_t kind);
std::tuple<int64_t, std::string> wgrad_current_algo(int64_t T, int64_t in, int64_t out,
                                                    int64_t kind);
at::Tensor mfma_test_32x32x16(at::Tensor A, at::Tensor B);
std::vector<at::Tensor> attn_tile_test_roundtrip(at::Tensor tile);
at::Tensor attn_tile_test_tr_fragments(at::Tensor tile, int64_t shape, int64_t nrows,
                                       int64_t buf);
at::Tensor attn_tile_test_pack_pair(at::Tensor x);
at::Tensor attn_tile_test_pack_frag16(at::Tensor x);
void fused_adamw(std::vector<at::Tensor> params, std::vector<at::Tensor> masters,
                 std::vector<at::Tensor> grads, std::vector<at::Tensor> exp_avg,
                 std::vector<at::Tensor> exp_avg_sq, double lr, double beta1, double beta2,
                 double eps, double weight_decay, double bias1, double bias2,
                 double grad_scale);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "lpp_amd gfx950 (MI355X/CDNA4) kernels";
  m.def("rmsnorm_fwd", &rmsnorm_fwd, "RMSNorm forward (y, invrms)");
  m.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm backward (dx, dw)");
  m.def("rmsnorm_bwd_fused", &rmsnorm_bwd_fused,
        "RMSNorm backward with the gradient adds fused: sums 1..3 partial dy (bf16 rounding "
        "after each add), adds dres to the rounded dx -> (dx_total, dw, dxT or empty)",
        py::arg("dys"), py::arg("x"), py::arg("weight"), py::arg("invrms"),
        py::arg("dres") = py::none(), py::arg("want_t") = false);
  m.def("rope_fwd", &rope_fwd, "RoPE forward");
  m.def("rope_bwd", &rope_bwd, "RoPE backward");
  m.def("rope_bwd_t", &rope_bwd_t,
        "RoPE backward that also writes dx^T [H*D, B*S] when aligned (D = 128, B*S % 64 == "
        "0, bf16): (dx, dxT), else (dx,)");
  m.def("swiglu_fwd", &swiglu_fwd, "SwiGLU forward");
  m.def("swiglu_bwd", &swiglu_bwd, "SwiGLU backward (dgate, dup)");
  m.def("swiglu_bwd_t", &swiglu_bwd_t,
        "SwiGLU backward that also writes dgate^T, dup^T [I, T] when aligned (T % 64 == 0, "
        "I % 128 == 0, bf16): (dgate, dup, dgateT, dupT), else (dgate, dup)");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused CE forward (loss_sum, lse, count)");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused CE backward (dlogits)");
  m.def("fused_adamw", &fused_adamw, "fused mixed-precision AdamW");
  m.def("attention_fwd", &attention_fwd, "flash causal attention forward (O, LSE2)");
  m.def("attention_bwd", &attention_bwd, "flash causal attention backward (dQ, dK, dV)");
  m.def("attention_fwd_docs", &attention_fwd_docs,
        "flash causal attention forward over packed rows (O, LSE2): query i sees keys "
        "doc_start[b][i] .. i; doc_start int32 [B,S]",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("doc_start"));
  m.def("attention_bwd_docs", &attention_bwd_docs,
        "flash causal attention backward over packed rows (dQ, dK, dV); doc_end[b][j] = one "
        "past the last token of key j's document, int32 [B,S]",
        py::arg("dO"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse2"), py::arg("doc_start"), py::arg("doc_end"));
  m.def("attention_set_block_order", &attention_set_block_order,
        "attention block order: 0 = legacy, 1 = XCD-balanced heavy-first (default, "
        "LPP_ATTN_ORDER)", py::arg("mode"));
  m.def("attention_get_block_order", &attention_get_block_order, "current order mode");
  m.def("attention_block_order", &attention_block_order,
        "host: [n,2] int (blk, head) of linear block ids 0..n-1; kind 0 fwd/dQ, 1 dK/dV",
        py::arg("kind"), py::arg("nblk"), py::arg("nheads"), py::arg("G"), py::arg("mode"));
  m.def("attention_time_kernel", &attention_time_kernel,
        "hipEvent ms per launch of one attention kernel (fwd|dq|dkdv) under an explicit "
        "block order; with doc_start and doc_end, of its packed-row instantiation",
        py::arg("kernel"), py::arg("dO"), py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("o"), py::arg("lse2"), py::arg("mode"), py::arg("G") = 0,
        py::arg("warmup") = 3, py::arg("reps") = 20, py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none());
  m.def("attention_decode", &attention_decode,
        "fused single-token decode: RoPE + KV-cache write + GQA attention over keys 0..p of "
        "each row's cache row -> o [N,1,H,128]; chunk 0 = the compiled-in chunk size",
        py::arg("q"), py::arg("k_new"), py::arg("v_new"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("cos"), py::arg("sin"), py::arg("positions"),
        py::arg("rows"), py::arg("lengths"), py::arg("uniform_pos"), py::arg("max_len"),
        py::arg("chunk") = 0);
  m.def("attention_decode_chunk", &attention_decode_chunk,
        "keys per workgroup of attention_decode");
  m.def("wgrad_f32_accum", &wgrad_f32_accum, "dW_f32 += dY^T @ X (hipBLASLt, beta=1)");
  m.def("wgrad_f32_accum_pre", &wgrad_f32_accum_pre,
        "dW_f32 += dyT @ xT^T, pre-transposed k-contiguous operands (hipBLASLt, beta=1)");
  m.def("transpose2d", &transpose2d, "bf16/fp16 [R,C] -> [C,R] LDS-tiled transpose");
  m.def("wgrad_bf16d_pre", &wgrad_bf16d_pre,
        "bf16-D pre-transposed wgrad GEMM into a reusable scratch (beta 0)");
  m.def("accum_bf16_f32", &accum_bf16_f32, "dst_f32 += src_bf16 (vectorised)");
  m.def("wgrad_tune", &wgrad_tune,
        "exhaustive hipBLASLt solution sweep for a wgrad shape -> [(index, ms, name)]",
        py::arg("T"), py::arg("in_dim"), py::arg("out"), py::arg("reps"), py::arg("kind") = 0);
  m.def("wgrad_set_algo", &wgrad_set_algo, "pin a hipBLASLt solution index for a shape",
        py::arg("T"), py::arg("in_dim"), py::arg("out"), py::arg("index"), py::arg("kind") = 0);
  m.def("wgrad_current_algo", &wgrad_current_algo,
        "current (heuristic-picked) solution for a shape -> (index, name)",
        py::arg("T"), py::arg("in_dim"), py::arg("out"), py::arg("kind") = 0);
  m.def("mfma_test_16x16x32", &mfma_test_16x16x32, "MFMA layout validation");
  m.def("mfma_test_32x32x16", &mfma_test_32x32x16, "MFMA 32x32x16 layout validation");
  m.def("attn_tile_test_roundtrip", &attn_tile_test_roundtrip,
        "attn_tile.h dual-use image: int16 [64,128] -> (tile by row reads, transpose by "
        "transposed reads) from one LDS image");
  m.def("attn_tile_test_tr_fragments", &attn_tile_test_tr_fragments,
        "attn_tile.h transposed reads: int16 [64,128] -> int16 [16,64,8], the B-fragments "
        "of MFMA shape 32 (frag = dt*4+ks) or 16 (frag = dt*2+half) as the kernels read them",
        py::arg("tile"), py::arg("shape"), py::arg("nrows") = 64, py::arg("buf") = 0);
  m.def("attention_lds_addresses", &attention_lds_addresses,
        "host: int32 [64] per-lane LDS byte addresses of one access pattern (stage | row | "
        "tr) of MFMA shape 32 or 16", py::arg("pattern"), py::arg("shape"), py::arg("idx"));
  m.def("attn_tile_test_pack_pair", &attn_tile_test_pack_pair,
        "attn_tile.h pack_pair: fp32 [32,32] in C layout -> int32 [64,2,4] A-fragment words");
  m.def("attn_tile_test_pack_frag16", &attn_tile_test_pack_frag16,
        "attn_tile.h pack_frag16: fp32 [32,16] in C layout -> int32 [64,4] A-fragment words");
}
