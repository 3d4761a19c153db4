/* implicit_abi.h -- the C ABI of csrc/implicit.hip: sample_pdf and emission-absorption raymarching.
 *
 * An extension of include/p3d_amd.h with a header and a prefix of its own: the entries of that header (p3d_*) are a closed set that
 * the ABI tests count and compare with the library's exports, so these entries are named p3di_* and declared here.  Same
 * conventions: extern "C", P3D_OK / P3D_ERR_* status codes, p3d_stream_t, no host sync.  pytorch3d_amd/_lib.py reads this file the
 * way it reads p3d_amd.h (EXTENSION_DECLARATIONS; _lib.call serves both tables). */
#ifndef P3D_AMD_IMPLICIT_ABI_H_
#define P3D_AMD_IMPLICIT_ABI_H_

#include "../../include/p3d_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SamplePdf by the contract of the reference's compiled CPU operator (sample_pdf/sample_pdf_cpu.cpp with its binary search), in place:
 * per row, partial[i] = the float32 running sum of weights[0..i] in index order, total = partial[n_bins-1] + eps; per sample u =
 * outputs[row, j]: v = total * u; i = the first index in [0, n_bins - 1) with !(partial[i] < v), n_bins - 1 if there is none
 * (std::lower_bound's halving steps, also on unordered sums); if i > 0, v -= partial[i-1]; then outputs[row, j] =
 *   bins[i+1] if v > weights[i];  else bins[i] + (v / weights[i]) * (bins[i+1] - bins[i]) if weights[i] > eps;  else bins[i],
 * in float32 without FMA and with the correctly rounded quotient.  bins (B, n_bins+1), weights (B, n_bins), outputs (B, S)
 * contiguous f32.  Every index stays in [0, n_bins): NaN or negative data gives wrong numbers, never an access outside the arrays.
 *
 * p3di_sample_pdf (device): a workgroup of 256 lanes takes P3D_SAMPLE_PDF_ROWS rows (fewer when they do not fit) with their running
 * sums in LDS at the odd row stride n_bins | 1.  A row whose stride passes P3D_SAMPLE_PDF_LDS_FLOATS (n_bins >= that number) has
 * its sums made by one lane per row in the workspace and is searched there by the same function: no n_bins is refused.  workspace:
 * p3di_sample_pdf_workspace_bytes(B, n_bins) bytes (0 for the LDS form, which takes NULL; smaller: P3D_ERR_WORKSPACE).
 * p3di_sample_pdf_host: the same loop on host pointers.  The two write the same bits.
 * B or S of 0: P3D_OK without a launch.  n_bins < 1, negative sizes, missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_SAMPLE_PDF_ROWS 16
#define P3D_SAMPLE_PDF_LDS_FLOATS 8192
size_t p3di_sample_pdf_workspace_bytes(int64_t B, int64_t n_bins);
int p3di_sample_pdf(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps,
                   void* workspace, size_t workspace_bytes, p3d_stream_t stream);
int p3di_sample_pdf_host(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps);

/* Emission-absorption raymarching (renderer/implicit/raymarching.py) over N rays of P points with C feature channels, in float32:
 *   x_k = one_plus_eps - d_k;   a_k = 1 for k < shift, else prod_{j <= k - shift} x_j;   w_k = d_k a_k;
 *   out[n, c] = sum_k w_k f_kc (c < C);   out[n, C] = 1 - prod_k (1 - d_k);   weights[n, k] = w_k when weights is not NULL.
 * densities (N, P), features (N, P, C), out (N, C+1), weights (N, P) contiguous f32.  C == 0 is the absorption-only raymarcher:
 * out (N, 1), features and weights unused.  shift >= P: a = 1 everywhere.
 * backward: grad_out (N, C+1), grad_weights (N, P) or NULL -> grad_densities (N, P), grad_features (N, P, C), every entry written:
 *   g_f_kc = w_k gF_c;   g_w_k = sum_c gF_c f_kc (+ grad_weights_k);
 *   g_d_k = a_k g_w_k - L_k T_k + gO prod_{j != k} (1 - d_j),   L_k = prod_{j < k} x_j,   T_k = g_w_{k+shift} d_{k+shift} + x_{k+1} T_{k+1}
 * -- no division, so a density of exactly 1 has its exact gradient.  Lanes run along the ray (segments of next_pow2(P) lanes up to
 * 64, then chunks of 64 with a carry); products and sums are shuffle scans and butterflies whose order P, C and shift fix: no atomic,
 * the same bits on every run and stream.  workspace (backward, P > 64 only): p3di_ea_raymarch_backward_workspace_bytes(N, P) bytes,
 * the prefix carries of every chunk (smaller: P3D_ERR_WORKSPACE).
 * N == 0: P3D_OK without a launch.  P < 1, shift < 1, negative sizes, missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
int p3di_ea_raymarch_forward(const float* densities, const float* features, int64_t N, int64_t P, int64_t C, int64_t shift,
                            float one_plus_eps, float* out, float* weights, p3d_stream_t stream);
size_t p3di_ea_raymarch_backward_workspace_bytes(int64_t N, int64_t P);
int p3di_ea_raymarch_backward(const float* densities, const float* features, const float* grad_out, const float* grad_weights,
                             int64_t N, int64_t P, int64_t C, int64_t shift, float one_plus_eps, float* grad_densities,
                             float* grad_features, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* P3D_AMD_IMPLICIT_ABI_H_ */
