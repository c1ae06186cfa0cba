/* libbuctd_hip.so - C ABI of the MI355X (gfx950) BUCTD hot path.
 *
 * The reference (amathislab/BUCTD) has no FFI on this path: every device op is
 * a torch.nn module call that lands in cuDNN / cuBLAS / ATen.  Each entry point
 * below names the reference call site it stands in for (file:line relative to
 * the reference root).  INTEGRATION.md shows the ctypes binding the Python host
 * (buctd_amd/_C.py) uses.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (buctd_last_error());
 *  - no allocation, no ownership transfer, no synchronisation: the caller owns
 *    all buffers (device pointers), passes a hipStream_t as `void* stream`, and
 *    kernels are only enqueued on that stream;
 *  - activations are fp32 NHWC  [N][H][W][C]; conv weights are fp32
 *    [Co][R][S][Ci] (physical layout of a torch channels_last OIHW tensor);
 *    Linear weights are [out][in]; token tensors are [B][T][C];
 *  - "rows" = product of all leading dims, "C" = innermost (channel) dim.
 */
#ifndef BUCTD_HIP_H
#define BUCTD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int buctd_version(void);
const char* buctd_last_error(void);

/* ------------------------------------------------------------------ conv --- */
typedef struct {
  int N, H, W, Ci; /* input  [N][H][W][Ci]            */
  int Co, R, S;    /* filter [Co][R][S][Ci]           */
  int stride, pad; /* symmetric                       */
  int Ho, Wo;      /* output [N][Ho][Wo][Co]          */
} buctd_conv_desc;

/* y = conv(x,w) (+bias) ; then, in this order and each optional:
 *   stats_partials != NULL : per-(row-group, channel) Welford partials (mean, M2) of the
 *                            biased conv output for train-mode BatchNorm (see buctd_bn_finalize);
 *   scale/shift   != NULL  : y = y*scale[c] + shift[c]   (eval-mode BatchNorm folded);
 *   residual      != NULL  : y += residual ; relu != 0 : y = max(y,0).
 * Replaces nn.Conv2d(+BatchNorm2d+ReLU+residual): pose_hrnet.py:28-98, pose_hrnet_coam.py:44-60,
 * nn.Linear on token tensors (R=S=1): self_attention.py:74-76,87. */
/* 1 when buctd_conv2d_fwd runs this shape on the thin-output kernel (stride-1 'same' 7x7 with <= 4 output channels: the
 * full-resolution preNet convolutions, pose_hrnet.py:431-442) - it then takes no fused epilogue: call it with bias
 * only and run buctd_bn_stats on the (3-channel) result for a train-mode BatchNorm. */
int buctd_conv2d_fwd_thin(const buctd_conv_desc* d);
int buctd_conv2d_fwd(const buctd_conv_desc* d, const float* x, const float* w, const float* bias,
                     const float* scale, const float* shift, const float* residual, int relu, float* y,
                     float* stats_partials, void* stream);
/* dx = conv_transpose(dy, w) (+bias, + Welford partials over dx): the data gradient of
 * buctd_conv2d_fwd, and the forward of nn.ConvTranspose2d (pose_resnet.py:197-205). */
int buctd_conv2d_dgrad(const buctd_conv_desc* d, const float* dy, const float* w, const float* bias, float* dx,
                       float* stats_partials, void* stream);
/* number / height of the Welford row groups written by fwd (transposed=0, channels=Co, rows=N*Ho*Wo)
 * or dgrad (transposed=1, channels=Ci, rows=N*H*W); partial buffer = ngroups*channels*2 floats. */
int buctd_conv2d_stats_groups(const buctd_conv_desc* d, int transposed, int* ngroups, int* rows_per_group);
/* dw (+)= sum over pixels dy (x) x ; split over pixels through `workspace`. */
size_t buctd_conv2d_wgrad_workspace(const buctd_conv_desc* d);
int buctd_conv2d_wgrad(const buctd_conv_desc* d, const float* x, const float* dy, float* dw, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);
/* What the three entry points above would launch for this descriptor: no launch, no device (the query and the launches call
 * the same routing functions).  direction: 0 buctd_conv2d_fwd, 1 buctd_conv2d_dgrad, 2 buctd_conv2d_wgrad.  flags: which
 * optional inputs the call passes (the routing reads nothing else of them); scale / residual / relu are forward only, a
 * weight gradient takes 0.  out[BUCTD_CONV_PLAN_INTS]:
 *   [0] route   0 = the implicit-GEMM kernel, else a thin-channel kernel of that direction:
 *               forward          1 / 2 four pixels per thread (<= 4 / a multiple of 8 input channels), 3 one pixel per
 *                                thread, 4 thin input (<= 4 channels -> 64, 3x3)
 *               data gradient    1 stride-2 thin dx, 2 thin on both sides, 3 four dx pixels per thread, 4 one per thread
 *               weight gradient  1 rolling rows (64 -> <= 3, 7x7), 2 tile kernel, 3 thin input
 *   route 0 only ([8] also for the thin weight gradients; everything else is 0 on a thin route):
 *   [1] tile id 0..10 (forward / data gradient) or weight-gradient configuration (0 = 64x64 scalar loads, 1..4 = 48 / 64 /
 *       96 / 128 x 64 vector loads)
 *   [2] BM  [3] BN  [4] WM  [5] MF    the workgroup tile, its wavefront rows and 16-row fragments per wavefront
 *   [6] vec    16-byte operand loads
 *   [7] par    stride-2 data gradient split into four output-parity classes
 *   [8] nsplit  [9] pix_per_split  [10] 1 = float4 slab reduction      (weight gradient)
 * Returns what the launch would return for a descriptor or a flag combination it refuses. */
#define BUCTD_CONV_BIAS 1
#define BUCTD_CONV_SCALE 2 /* scale and shift */
#define BUCTD_CONV_RESIDUAL 4
#define BUCTD_CONV_RELU 8
#define BUCTD_CONV_STATS 16
#define BUCTD_CONV_PLAN_INTS 11
int buctd_conv2d_plan(const buctd_conv_desc* d, int direction, int flags, int* out);

/* 3x3 / stride 1 / pad 1 convolution on the bf16 matrix cores with split-fp32 operands, fp32 accumulate
 * (csrc/conv3x3.hip).  Replaces the BasicBlock convs of pose_hrnet.py:28-57 (nn.Conv2d(k=3, s=1, p=1, bias=False)
 * forward and its autograd data gradient).  Same epilogue options as buctd_conv2d_fwd.  Two families of entry points:
 *   buctd_conv3x3_bf16x6_*  fp32-class (the engine's default): x = h + m + l exactly (three bf16 pieces), six MFMAs
 *                           per product; dropped piece products are <= 2^-24 of the product;
 *   buctd_conv3x3_bf16x3_*  optional reduced precision: two pieces, three MFMAs, ~2^-16 per product.
 *
 * The filter is consumed as a prepared image (bf16 pieces in the kernel's stage order), produced once per
 * weight update by the family's _prep from the forward filter w = [Co][3][3][Ci]:
 *   flip = 0: image for the forward convolution (Ci -> Co);
 *   flip = 1: image for its data gradient (the call below then takes x = dy [N][H][W][Co] with "Ci" = Co and
 *             produces y = dx [N][H][W][Ci] with "Co" = Ci).
 * A prepared image belongs to the family that made it.
 * stats_counts: ngroups ints (valid rows per group; pad positions of the flattened tile are skipped). */
int buctd_conv3x3_bf16x6_supported(int N, int H, int W, int Ci, int Co);
int buctd_conv3x3_bf16x6_stats_groups(int N, int H, int W, int Ci, int Co, int* ngroups, int* rows_per_group);
size_t buctd_conv3x3_bf16x6_prep_bytes(int Ci, int Co, int flip);
int buctd_conv3x3_bf16x6_prep(int Ci, int Co, const float* w, int flip, void* wprep, void* stream);
int buctd_conv3x3_bf16x6(int N, int H, int W, int Ci, int Co, const float* x, const void* wprep, const float* bias,
                         const float* scale, const float* shift, const float* residual, int relu, float* y,
                         float* stats_partials, int* stats_counts, void* stream);
/* The accumulator forms (see "BatchNorm statistics without finalize launches" below).
 * _acc: forward convolution whose output statistics are added to stats_acc (NULL: none) and whose input may be the raw
 * output z of the producing convolution, normalised while it is staged with THAT layer's statistics decoded from its
 * accumulator (in_bn != NULL: with in_gamma / in_beta / in_relu, [Ci] arrays): the kernel convolves
 * relu((z - mean) * (invstd * gamma) + beta) - bitwise what buctd_bn_apply would have written - so the tensor between
 * bn1/relu and conv2 of a BasicBlock (pose_hrnet.py:44-49) never exists in HBM.  The launch's first tile writes mean / invstd
 * out and updates the running statistics.
 * _bnstat_acc: data gradient of a 3x3 convolution (buctd_conv3x3_bf16x6 on the flip = 1 image; residual = the skip gradient,
 * NULL ok) that also forms the REDUCTION pass of the BatchNorm backward consuming its output g = y: s1 = sum m g,
 * s2 = sum m g (z - mean) invstd, with m the ReLU mask of that BatchNorm's forward output (bn_y > 0 where given, else rebuilt
 * from bn_z as (z - mean)(invstd gamma) + beta > 0), added to the accumulator bn_acc - the input of buctd_bn_bwd_acc.  What
 * autograd does with three more passes over g, z and y (the sum reductions of native_batch_norm_backward,
 * pose_hrnet.py:41-57). */
struct buctd_bn_acc_in_;
int buctd_conv3x3_bf16x6_acc(int N, int H, int W, int Ci, int Co, const float* x, const void* wprep, const float* residual,
                             int relu, float* y, void* stats_acc, const struct buctd_bn_acc_in_* in_bn, const float* in_gamma,
                             const float* in_beta, int in_relu, void* stream);
int buctd_conv3x3_bf16x6_bnstat_acc(int N, int H, int W, int Ci, int Co, const float* x, const void* wprep,
                                    const float* residual, float* y, const float* bn_z, const float* bn_y,
                                    const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                    void* bn_acc, void* stream);
/* Several independent 3x3 convolutions in ONE launch - the k-th convolutions of the 2-4 branches of a HighResolutionModule
 * (pose_hrnet.py:177-185), which cost the same FLOPs on maps of different size.  The tiles of all of them form one grid
 * (costliest first), so the launch is several rounds of workgroups that de-phase instead of one phase-locked round per
 * convolution.  Each entry is one buctd_conv3x3_bf16x6_acc call (forward: stats_acc / in_bn ...) or one
 * buctd_conv3x3_bf16x6_bnstat_acc call (data gradient: bn_acc != NULL with bn_z ...; without bn_acc a plain data gradient);
 * results are bit-identical to those calls.  n <= 4. */
typedef struct {
  int N, H, W, Ci, Co;
  const float* x;
  const void* wprep;
  const float* residual;
  int relu;
  float* y;
  void* stats_acc;                         /* forward statistics of y (NULL: none) */
  const struct buctd_bn_acc_in_* in_bn;    /* input BatchNorm from the producer's accumulator (NULL: none) */
  const float *in_gamma, *in_beta;
  int in_relu;
  const float *bn_z, *bn_y, *bn_mean, *bn_invstd, *bn_gamma, *bn_beta;   /* BatchNorm-backward by-product ... */
  void* bn_acc;                                                          /* ... into this accumulator (NULL: none) */
} buctd_c3_conv;
int buctd_conv3x3_bf16x6_group(int n, const buctd_c3_conv* convs, void* stream);
/* The same for EVAL mode (validate(), lib/core/function.py:178-336; inference): the k-th convolutions of the branches with the
 * folded BatchNorm (y = conv * scale + shift), the skip connection and the ReLU in the epilogue - each entry is one
 * buctd_conv3x3_bf16x6(N, H, W, Ci, Co, x, wprep, NULL, scale, shift, residual, relu, y, NULL, NULL, stream) call, bit-identical
 * to it; members that share no kernel go out one launch each.  n <= 4. */
typedef struct {
  int N, H, W, Ci, Co;
  const float* x;
  const void* wprep;
  const float *scale, *shift;     /* both or neither */
  const float* residual;
  int relu;
  float* y;
} buctd_c3_conv_eval;
int buctd_conv3x3_bf16x6_group_eval(int n, const buctd_c3_conv_eval* convs, void* stream);
/* Train-mode launches (the option sets of block.hip: statistics accumulator, input BatchNorm from an accumulator, skip
 * gradient, BatchNorm-backward sums) run kernels specialised on the option set (csrc/conv3x3_lean.hip). */
/* The number of workgroups buctd_conv3x3_bf16x6_group(n, convs) launches as ONE kernel (0: the members share no kernel and go
 * out one launch each; < 0: error).  No launch - for tools that find a launch in a kernel trace by its grid (bench.py). */
int buctd_conv3x3_bf16x6_group_workgroups(int n, const buctd_c3_conv* convs);
/* What buctd_conv3x3_bf16x6_group(n, convs) would launch (host code only, no launch; the answer is the descriptor the launch
 * hands to its kernel).  Nothing is read through the tensor pointers; x, wprep and y must be non-NULL and the optional ones set
 * as in the call, since which of them are set decides the option set.  Entries with none of stats_acc / in_bn / residual /
 * relu / bn_acc are what buctd_conv3x3_bf16x6_group_eval makes of its entries: n > 1 of them give the plan of that call.
 * out[BUCTD_C3_GROUP_PLAN_INTS]: [0] 1 = one kernel, 0 = one launch per member (then all that follows but [5] is -1);
 * [1] the train-mode option set (C3M_* mask), -1 = the general group kernel; [2] kernel family; [3] grid (workgroups);
 * [4] dynamic LDS bytes; [5] n; then per member IN LAUNCH ORDER (costliest tile first) six values from [6 + 6 i]: its index in
 * convs, variant (index into the family's tile table), gx (position tiles), gy (column tiles), tiles = gx * gy, col_major. */
#define BUCTD_C3_GROUP_PLAN_INTS 30
int buctd_conv3x3_bf16x6_group_plan(int n, const buctd_c3_conv* convs, int* out);
/* Which tile plan and which kernel a bf16x6 launch of this shape takes (host code only, no launch; computed by the functions
 * the launch itself goes through, so the answer cannot drift from it).  option_set: the train-mode option set of the launch
 * as the C3M_* mask of csrc/c3_lean.h - 2 STATS (_acc with stats_acc), 3 STATS | IN_BN (+ in_bn), 8 BS_REBUILD (_bnstat_acc,
 * bn_y == NULL), 20 RES | BS_Y (_bnstat_acc with residual and bn_y), 4 RES (plain data gradient with residual) - or -1 for
 * every other call (bias, eval scale / shift, ReLU, partial-sum statistics, nothing at all).
 * out[11] = MF, NF, WM, WN (16-row / 16-column fragments per wave, waves along positions / columns), single A buffer (the
 * 448- / 512-position tiles), column-major tile order, kernel (0 = conv3x3_x6_kernel, 1 = the train-mode kernel of the option
 * set), its kernel family and variant index (-1, -1 for kernel 0), BM, BN (positions / columns of a workgroup tile).
 * BUCTD_EINVAL: unsupported shape or option set.  For tests that must know which code path a shape exercises. */
int buctd_conv3x3_bf16x6_plan(int N, int H, int W, int Ci, int Co, int option_set, int* out);
int buctd_conv3x3_bf16x3_supported(int N, int H, int W, int Ci, int Co);
int buctd_conv3x3_bf16x3_stats_groups(int N, int H, int W, int Ci, int Co, int* ngroups, int* rows_per_group);
size_t buctd_conv3x3_bf16x3_prep_bytes(int Ci, int Co, int flip);
int buctd_conv3x3_bf16x3_prep(int Ci, int Co, const float* w, int flip, void* wprep, void* stream);
/* The same for n filters in ONE launch (every prepared image of a model after an optimizer step), either family:
 * item.reserved = 3 writes the bf16x6 image, anything else the bf16x3 one.  `items_device` is an array in device
 * memory; an item has steps * Nc * 8 pieces (= prep_bytes / 16 for bf16x3, / 24 for bf16x6); piece_begin is the running
 * sum over the preceding items and total_pieces the sum over all of them. */
typedef struct {
  const float* w;       /* forward filter [Co][3][3][Ci] */
  void* wprep;          /* destination image */
  int Ci, Co, flip, reserved;
  long piece_begin;
} buctd_c3_prep_item;
int buctd_conv3x3_bf16x3_prep_batched(const buctd_c3_prep_item* items_device, int n, long total_pieces, void* stream);
int buctd_conv3x3_bf16x3(int N, int H, int W, int Ci, int Co, const float* x, const void* wprep, const float* bias,
                         const float* scale, const float* shift, const float* residual, int relu, float* y,
                         float* stats_partials, int* stats_counts, void* stream);

/* weight gradient of the same convolution on the bf16 matrix cores (autograd of nn.Conv2d, pose_hrnet.py:28-57;
 * transpose-read fragments from position-major LDS tiles, split over positions through `workspace`):
 * dw (+)= sum_p dy[p] (x) x[p + tap].  dw: [Co][3][3][Ci].  Families as above. */
int buctd_conv3x3_wgrad_bf16x6_supported(int N, int H, int W, int Ci, int Co);
/* the plan of that launch (no launch): out[4] = CF (3: 48-channel chunk pairs, 2: 32-channel), nsplit (position splits per
 * chunk pair), q, rem (a split takes q stages, the first rem of them q + 1).  BUCTD_EINVAL: unsupported shape. */
int buctd_conv3x3_wgrad_bf16x6_plan(int N, int H, int W, int Ci, int Co, int* out);
size_t buctd_conv3x3_wgrad_bf16x6_workspace(int N, int H, int W, int Ci, int Co);
int buctd_conv3x3_wgrad_bf16x6(int N, int H, int W, int Ci, int Co, const float* x, const float* dy, float* dw,
                               int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* the weight gradient with the on-the-fly BatchNorm(+ReLU) of buctd_conv3x3_bf16x6_acc applied to its X operand (x = the
 * producer's raw output z), from the [Ci] arrays x_mean / x_invstd that forward launch wrote out */
int buctd_conv3x3_wgrad_bf16x6_bnin(int N, int H, int W, int Ci, int Co, const float* x, const float* dy, float* dw,
                                    int accumulate, const float* x_mean, const float* x_invstd, const float* x_gamma,
                                    const float* x_beta, int x_relu, void* workspace, size_t workspace_bytes,
                                    void* stream);
/* The weight gradients of the k-th convolutions of the 2-4 branches of a HighResolutionModule (pose_hrnet.py:177-185) in ONE
 * launch (+ one for their slab reductions).  Convolutions that share a launch fill the chip together, so each is cut into
 * fewer position splits than it would be alone: less halo re-reading, fewer slabs (a different, still fixed, summation order
 * than the single call: deterministic, fp32-class, not bit-identical to it).  Each item needs its OWN workspace of
 * buctd_conv3x3_wgrad_bf16x6_group_workspace(n, ...) bytes (n = convolutions in the launch); x_mean != NULL: the BatchNorm
 * (+ReLU) of the producer applied to x while it is staged, as in buctd_conv3x3_wgrad_bf16x6_bnin.  n <= 4. */
typedef struct {
  int N, H, W, Ci, Co;
  const float *x, *dy;
  float* dw;
  int accumulate;
  const float *x_mean, *x_invstd, *x_gamma, *x_beta;
  int x_relu;
  void* workspace;
  size_t workspace_bytes;
} buctd_wg3_conv;
size_t buctd_conv3x3_wgrad_bf16x6_group_workspace(int n, int N, int H, int W, int Ci, int Co);
int buctd_conv3x3_wgrad_bf16x6_group(int n, const buctd_wg3_conv* convs, void* stream);
/* workgroups of the weight-gradient kernel that call launches (no launch; tools that search a kernel trace by grid: bench.py) */
int buctd_conv3x3_wgrad_bf16x6_group_workgroups(int n, const buctd_wg3_conv* convs);
/* What that call would launch (host code only, no launch; tensors and workspaces may be NULL; from the descriptors the launch
 * builds).  out[BUCTD_WG3_GROUP_PLAN_INTS]: per member eight values from [8 k]: CF, nsplit, q, rem (as
 * buctd_conv3x3_wgrad_bf16x6_plan, for the member's share of the group), its first workgroup, its chunk pairs, its first chunk
 * pair in the reduction launch, the bytes of its workspace the launch writes; unused members -1.  [32] workgroups of the
 * launch, [33] dynamic LDS bytes.  Mixed chunk widths: BUCTD_EINVAL, as the launch. */
#define BUCTD_WG3_GROUP_PLAN_INTS 34
int buctd_conv3x3_wgrad_bf16x6_group_plan(int n, const buctd_wg3_conv* convs, int* out);
int buctd_conv3x3_wgrad_bf16x3_supported(int N, int H, int W, int Ci, int Co);
size_t buctd_conv3x3_wgrad_bf16x3_workspace(int N, int H, int W, int Ci, int Co);
int buctd_conv3x3_wgrad_bf16x3(int N, int H, int W, int Ci, int Co, const float* x, const float* dy, float* dw,
                               int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- matmul --- */
typedef struct {
  int batch, M, N, K;
  int a_layout;            /* 0: A(m,k)=A[m*lda + (k/Kc)*group_stride_a + k%Kc] ; 1: A(m,k)=A[k*lda+m]   */
  int b_layout;            /* 0: B(k,n)=B[n*ldb + (k/Kc)*group_stride_bk + k%Kc] ;
                              1: B(k,n)=B[k*ldb + (n/Nc)*group_stride_bn + n%Nc]                          */
  int lda, ldb, ldc;       /* C(m,n)=C[m*ldc + (n/Nc)*group_stride_c + n%Nc]                              */
  long stride_a, stride_b, stride_c; /* per-batch element strides (0 = shared operand) */
  int Kc; long group_stride_a, group_stride_bk;
  int Nc; long group_stride_bn, group_stride_c;
  float alpha;
  int bias_axis;           /* 0: bias[n], 1: bias[m] (only read when bias != NULL) */
} buctd_matmul_desc;
/* C = alpha*A*B (+bias). Replaces torch.matmul / nn.Linear in self_attention.py:78,86,150,158-159. */
size_t buctd_matmul_workspace(const buctd_matmul_desc* d);
int buctd_matmul(const buctd_matmul_desc* d, const float* A, const float* B, const float* bias, float* C,
                 void* workspace, size_t workspace_bytes, void* stream);
/* What buctd_matmul would launch for this descriptor and these operand pointers: no launch, no device (the query and the
 * launch call the same routing function).  A and B count only for their alignment (16-byte operand loads need 16-byte
 * aligned pointers) and are never dereferenced.  out[BUCTD_MATMUL_PLAN_INTS]:
 *   [0] tile id   0 = 128x64 scalar loads, 1 = 128x48, 2 = 128x96, 3 = 128x128 (16-byte loads)
 *   [1] BM  [2] BN  [3] WM  [4] MF    the workgroup tile, its wavefront rows and 16-row fragments per wavefront
 *   [5] vec    16-byte operand loads
 *   [6] nsplit  [7] k_per_split       split-K: nsplit > 1 needs buctd_matmul_workspace(d) = batch*nsplit*M*N*4 bytes
 * Returns what buctd_matmul would return for a descriptor it refuses. */
#define BUCTD_MATMUL_PLAN_INTS 8
int buctd_matmul_plan(const buctd_matmul_desc* d, const void* A, const void* B, int* out);

/* ------------------------------------------------------------- batchnorm --- */
/* Combine Welford partials -> mean, invstd (biased var, eps) and update running stats
 * (momentum, unbiased var) exactly like nn.BatchNorm2d in train mode (pose_hrnet.py:37).
 * group_counts (NULL ok): valid rows of each group when they are not rows_per_group-regular. */
int buctd_bn_finalize(const float* partials, const int* group_counts, int ngroups, int rows_per_group, long rows,
                      int C, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                      float* running_var, void* stream);
/* Welford partials of a plain [rows][C] tensor (when the producer was not a conv epilogue). */
int buctd_bn_stats(const float* z, long rows, int C, float* partials, int* ngroups, int* rows_per_group,
                   void* stream);
int buctd_bn_stats_groups(long rows, int C, int* ngroups, int* rows_per_group);
/* y = act((z-mean)*invstd*gamma+beta (+residual)) */
int buctd_bn_apply(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                   const float* residual, int relu, float* y, long rows, int C, void* stream);
/* Backward of bn_apply in train mode. y is the forward output (ReLU mask), may be NULL when relu==0.  With relu != 0
 * and y == NULL the mask is rebuilt bit-exactly from z as (z-mean)*(invstd*gamma)+beta > 0 - valid only when the
 * forward had no residual - which saves one full read of the activation tensor per pass (beta is read only then).
 * Writes dz; dres (NULL ok) receives the masked upstream gradient (gradient of the residual input);
 * dgamma/dbeta are overwritten (accumulate=0) or added to. workspace: buctd_bn_bwd_workspace bytes. */
size_t buctd_bn_bwd_workspace(long rows, int C);
int buctd_bn_bwd(const float* dy, const float* y, const float* z, const float* mean, const float* invstd,
                 const float* gamma, const float* beta, int relu, long rows, int C, float* dz, float* dres,
                 float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The rest of buctd_bn_bwd when the reduction pass already happened: part = [nparts][2][C] partial (s1, s2) sums over any
 * grouping of the rows, from any producer (the sums buctd_bn_bwd's own reduction forms per row range) -> fp64 merge,
 * dgamma / dbeta, then dz (and dres).  workspace: 2 * C floats. */
int buctd_bn_bwd_from_partials(const float* dy, const float* y, const float* z, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, int relu, long rows, int C, const float* part,
                               int nparts, float* dz, float* dres, float* dgamma, float* dbeta, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream);
/* ---- BatchNorm statistics without finalize launches (csrc/bn_acc.h) ----
 * The kernel that produces a tensor reduces it to one pair of sums per workgroup and channel and adds the pair into an
 * ACCUMULATOR with integer atomics (fixed point, two 64-bit limbs per sum: order-independent, so bit-deterministic); the
 * kernel that consumes the statistics decodes two numbers per channel in its prologue.  Nothing is launched between the
 * two (the mean/var reduction of native_batch_norm and the sum reductions of native_batch_norm_backward,
 * pose_hrnet.py:41-57, as by-products of their neighbours).  An accumulator is buctd_bn_acc_bytes(C) bytes and must be ZERO
 * when its producer is launched.
 * buctd_bn_acc_in: how a consumer takes FORWARD statistics from an accumulator holding (sum z, sum z^2) over `rows` values per
 * channel: it derives mean / invstd (biased variance, eps) itself; ONE workgroup of the launch also writes them to
 * mean_out / invstd_out ([C] each: what the backward kernels read) and updates running_mean / running_var (NULL: not
 * tracked) with `momentum` and the unbiased variance, like nn.BatchNorm2d in train mode. */
size_t buctd_bn_acc_bytes(int C);
typedef struct buctd_bn_acc_in_ {
  const void* acc;
  long rows;
  float eps, momentum;
  float *mean_out, *invstd_out;
  float *running_mean, *running_var;
} buctd_bn_acc_in;
/* buctd_bn_apply with the statistics taken from an accumulator (C % 4 == 0) */
int buctd_bn_apply_acc(const float* z, const buctd_bn_acc_in* st, const float* gamma, const float* beta,
                       const float* residual, int relu, float* y, long rows, int C, void* stream);
/* buctd_bn_bwd on an accumulator of the backward sums (sum g, sum g zhat): acc_ready = 0 runs the streaming reduction into
 * `acc` (zero on entry) first; acc_ready = 1: the data gradient that produced dy already filled it
 * (buctd_conv3x3_bf16x6_bnstat_acc).  The apply kernel decodes the sums and writes dgamma / dbeta.  C % 4 == 0, C <= 1024. */
int buctd_bn_bwd_acc(const float* dy, const float* y, const float* z, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, int relu, long rows, int C, float* dz, float* dres,
                     float* dgamma, float* dbeta, int accumulate, void* acc, int acc_ready, void* stream);
/* The same for the 2-4 branch tensors of a HighResolutionModule (pose_hrnet.py:177-185) in ONE launch per kernel kind: every
 * tensor is processed exactly as by its own buctd_bn_apply_acc / buctd_bn_bwd_acc call (bit-identical results).  n <= 4. */
typedef struct {
  const float* z;
  buctd_bn_acc_in st;
  const float *gamma, *beta, *residual;
  int relu;
  float* y;
  long rows;
  int C;
} buctd_bn_apply_item;
int buctd_bn_apply_acc_group(int n, const buctd_bn_apply_item* items, void* stream);
typedef struct {
  const float *dy, *y, *z, *mean, *invstd, *gamma, *beta;
  int relu;
  long rows;
  int C;
  float *dz, *dres, *dgamma, *dbeta;
  int accumulate;
  void* acc;
  int acc_ready;
} buctd_bn_bwd_item;
int buctd_bn_bwd_acc_group(int n, const buctd_bn_bwd_item* items, void* stream);
/* eval-mode helpers: scale = gamma/sqrt(var+eps), shift = beta - mean*scale */
int buctd_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                  float eps, int C, float* scale, float* shift, void* stream);

/* ----------------------------------------------------------- elementwise --- */
/* out[i] = a[i] + b[i] (b may be NULL -> copy); relu optional */
int buctd_add(const float* a, const float* b, float* out, long n, int relu, void* stream);
/* out = terms[0] + ... + terms[n-1] (2 <= n <= 4, host array of device pointers), summed left to right: the gradient
 * fan-in of a tensor with several consumers (HRNet fuse rows, pose_hrnet.py:257-265) in one pass */
int buctd_add_n(const float* const* terms, int n, float* out, long count, void* stream);
/* out[i] = a[i] * b[i]: DAModule with MODEL.ATT_CHANNEL_ONLY, `input * c_out` (pose_hrnet_coam.py:716-717) */
int buctd_mul(const float* a, const float* b, float* out, long n, void* stream);
/* out[i] = x[i] * alpha * (*dev_scalar) ; dev_scalar is a device pointer or NULL (chain rule through
 * the scalar loss without a host sync: loss.backward() hands d(loss) over as a device scalar) */
int buctd_scale(const float* x, const float* dev_scalar, float alpha, float* out, long n, void* stream);
/* dst[r][cd0+c] = src[r][cs0+c] for c < Cc: channel concat / split on [rows][C] tensors
 * (torch.cat((x, x_cond), dim=1), transpose_h.py:672) */
int buctd_copy_channels(const float* src, long rows, int Cs, int cs0, float* dst, int Cd, int cd0, int Cc,
                        void* stream);
/* out[b][i] = a[b][i] + v[i]: position embedding added to each image's tokens (transpose_h.py:189-192) */
int buctd_add_bcast(const float* a, const float* v, float* out, long batch, long n, void* stream);
/* out[i] (+)= sum over b of x[b*n + i], b ascending; accumulate != 0 adds to what out holds (out first, then
 * b = 0..batch-1): gradient of a learnable position embedding.  One thread per output, no atomics: bit-reproducible,
 * and the 16-byte path (n % 4 == 0, aligned pointers) returns the bits of the scalar one.  x and out must not overlap. */
int buctd_batch_sum(const float* x, long batch, long n, float* out, int accumulate, void* stream);
/* dx = dy * (y > 0) */
int buctd_relu_bwd(const float* dy, const float* y, float* dx, long n, void* stream);
/* column sums of [rows][C] (bias gradients); db overwritten or accumulated */
size_t buctd_colsum_workspace(long rows, int C);
int buctd_colsum(const float* x, long rows, int C, float* out, int accumulate, void* workspace,
                 size_t workspace_bytes, void* stream);
/* NCHW channel slice [c0, c0+Cc) of x[N][Ctot][H][W]  ->  NHWC [N][H][W][Cc], and back (full tensor). */
int buctd_nchw_to_nhwc(const float* x, int N, int Ctot, int c0, int Cc, int H, int W, float* y, void* stream);
int buctd_nhwc_to_nchw(const float* x, int N, int C, int H, int W, float* y, void* stream);
/* HighResolutionModule fuse (pose_hrnet.py:250-265): out = relu(sum_j upsample_nearest(term_j, 2^shift_j)).
 * terms[j] is [N][H>>shift_j][W>>shift_j][C]; up to 4 terms. */
int buctd_fuse_sum(const float* const* terms, const int* shifts, int nterms, int N, int H, int W, int C, int relu,
                   float* out, void* stream);
/* gradient of one fuse term: g[n][h][w][c] = sum over its 2^shift x 2^shift block of dy*(y>0) (y NULL: no mask) */
int buctd_fuse_sum_bwd(const float* dy, const float* y, int shift, int N, int H, int W, int C, float* g,
                       void* stream);
/* torchvision TF.resize (bilinear, align_corners=False, no antialias; pose_hrnet_coam.py:755) of the NCHW
 * channel slice [c0, c0+Cc) of x -> NHWC [N][Ho][Wo][Cc] */
int buctd_resize_bilinear(const float* x, int N, int Ctot, int c0, int Cc, int H, int W, int Ho, int Wo, float* y,
                          void* stream);
/* MaxPool2d(3, stride 2, pad 1) NHWC (pose_resnet.py:122) forward (argmax index saved) / backward */
int buctd_maxpool3x3s2_fwd(const float* x, int N, int H, int W, int C, float* y, int32_t* idx, void* stream);
int buctd_maxpool3x3s2_bwd(const float* dy, const int32_t* idx, int N, int H, int W, int C, float* dx,
                           void* stream);

/* ------------------------------------------------------------- attention --- */
/* Row softmax with fused scale and inverted dropout (self_attention.py:78-84):
 *   p = softmax(scale * s) over the last dim (length L);  pd = p * keep / (1-p_drop),
 *   keep drawn from a counter-based generator keyed by (seed, row, col) so the backward can rebuild it.
 * p (pre-dropout) and pd may alias when p_drop == 0. */
int buctd_softmax_dropout_fwd(const float* s, long rows, int L, float scale, float p_drop, uint64_t seed, float* p,
                              float* pd, void* stream);
/* ds = scale * p * (g - sum_j g_j p_j), g = dpd * keep/(1-p_drop) */
int buctd_softmax_dropout_bwd(const float* dpd, const float* p, long rows, int L, float scale, float p_drop,
                              uint64_t seed, float* ds, void* stream);
/* Device-seed forms (_dseed) of the dropout entries: the same signature with `const uint64_t* seed` in place of the value -
 * the kernels read *seed once, at start, so a captured step graph draws fresh masks per replay (engine.StepGraph,
 * fresh_dropout_masks=True).  Output equals the value entry's with seed = *seed, bit for bit.  Same reference call sites. */
int buctd_softmax_dropout_fwd_dseed(const float* s, long rows, int L, float scale, float p_drop, const uint64_t* seed,
                                    float* p, float* pd, void* stream);
int buctd_softmax_dropout_bwd_dseed(const float* dpd, const float* p, long rows, int L, float scale, float p_drop,
                                    const uint64_t* seed, float* ds, void* stream);
/* Fused position attention for narrow query/key contractions (self_attention.py:74-86 with fc_q folded into the
 * keys: logits = scale * q' k'^T with q' = [y_cond, 1, 0-pad] and k' = fc_k(y) [Wq | bq | 0], both [B][T][R4]).
 * out = dropout(softmax(logits)) v, v and out [B][T][C]; nothing of size T x T is written to memory.
 * m / linv [B][T] receive the row max and reciprocal row sum (saved for the backward).  The dropout mask is a
 * counter hash of (seed, b*T + i, j), rebuilt by the backward.  Shapes: T % 64 == 0, R4 in {4,8,16,20},
 * C in {16,32,48,64,96,128,192} (buctd_attn_smallqk_supported).  bf16x3 != 0 selects the variants whose T- and
 * C-contractions run on the bf16 matrix cores with split-fp32 operands: 1 = two pieces per operand (accuracy class of
 * buctd_conv3x3_bf16x3), 2 = three pieces, six MFMAs per product (fp32 class, as buctd_conv3x3_bf16x6; C <= 128).
 * R4 <= 8 only; wider contractions silently use the fp32 kernels. */
int buctd_attn_smallqk_supported(int T, int R4, int C);
/* What buctd_attn_smallqk_fwd / _bwd (dseed = 0) or their _dseed forms (dseed != 0) would launch for these arguments: no
 * launch, no device (the query and the launches call the same routing function).  flag is their bf16x3 argument.
 * out[BUCTD_ATTN_SMALLQK_PLAN_INTS]:
 *   [0] kernel family   0 = fp32 MFMA kernels, 1 = split-bf16 kernels
 *   [1] R4  [2] CF = C / 16       the template arguments of the family's kernels
 *   [3] bf16 pieces per operand   0 (fp32 family), 2 or 3
 *   [4] the forward runs the separate statistics pass (the split forward keeps the statistics itself)
 *   [5] DROP   [6] DSEED          dropout kernels; seed read from device memory (without dropout: the value kernels)
 * Returns what the launches return for a shape or p_drop they refuse (out is then all zero). */
#define BUCTD_ATTN_SMALLQK_PLAN_INTS 7
int buctd_attn_smallqk_plan(int T, int R4, int C, int flag, float p_drop, int dseed, int* out);
int buctd_attn_smallqk_fwd(int B, int T, int R4, int C, const float* q, const float* k, const float* v, float scale,
                           float p_drop, uint64_t seed, int bf16x3, float* out, float* m, float* linv, void* stream);
/* dq/dk: [B][T][R4] gradients of q'/k'; dv: [B][T][C]; dvec_workspace: B*T floats. */
int buctd_attn_smallqk_bwd(int B, int T, int R4, int C, const float* q, const float* k, const float* v,
                           const float* o, const float* dout, const float* m, const float* linv, float scale,
                           float p_drop, uint64_t seed, int bf16x3, float* dq, float* dk, float* dv,
                           float* dvec_workspace, void* stream);
/* device-seed forms (self_attention.py:74-86 in a captured training step) */
int buctd_attn_smallqk_fwd_dseed(int B, int T, int R4, int C, const float* q, const float* k, const float* v, float scale,
                                 float p_drop, const uint64_t* seed, int bf16x3, float* out, float* m, float* linv,
                                 void* stream);
int buctd_attn_smallqk_bwd_dseed(int B, int T, int R4, int C, const float* q, const float* k, const float* v,
                                 const float* o, const float* dout, const float* m, const float* linv, float scale,
                                 float p_drop, const uint64_t* seed, int bf16x3, float* dq, float* dk, float* dv,
                                 float* dvec_workspace, void* stream);
/* elementwise inverted dropout (transpose_h.py:180-183), mask rebuilt from (seed, index) */
int buctd_dropout(const float* x, float* y, long n, float p_drop, uint64_t seed, void* stream);
int buctd_dropout_dseed(const float* x, float* y, long n, float p_drop, const uint64_t* seed, void* stream);
/* The device form of the host's dropout seed stream (ops.next_seed, the step-graph replay of
 * lib/core/function.py:102-175): table[i] = base * 0x9E3779B97F4A7C15 + (counter0 + i + 1) * 0xD1B54A32D192ED03 (mod 2^64),
 * the seed of the (i + 1)-th draw after draw number counter0. */
int buctd_dropout_seed_fill(uint64_t* table, int n, uint64_t base, uint64_t counter0, void* stream);
/* LayerNorm over the last dim (transpose_h.py:178-179) */
int buctd_layernorm_fwd(const float* x, const float* gamma, const float* beta, long rows, int C, float eps, float* y,
                        float* mean, float* invstd, void* stream);
/* LayerNorm(a + b) in one pass (the post-norm residual of the encoder layer, transpose_h.py:204-209); sum_out (NULL ok)
 * receives a + b - the tensor buctd_layernorm_bwd takes as x. */
int buctd_add_layernorm_fwd(const float* a, const float* b, const float* gamma, const float* beta, long rows, int C, float eps,
                            float* sum_out, float* y, float* mean, float* invstd, void* stream);
size_t buctd_layernorm_bwd_workspace(long rows, int C);
int buctd_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma,
                        long rows, int C, float* dx, float* dgamma, float* dbeta, int accumulate, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------- loss / target / decode --- */
/* JointsMSELoss (core/loss.py:23-41): loss = 0.5/(K*N*HW) * sum w^2 (p-g)^2 ; grad (NULL ok) = dloss/dp * gscale.
 * pred/gt are [N][K][HW] (NCHW heatmaps), w is [N][K] (NULL: weights 1). workspace: N*K floats. */
int buctd_joints_mse(const float* pred, const float* gt, const float* w, int N, int K, int HW, float* loss,
                     float* grad, float gscale, void* workspace, size_t workspace_bytes, void* stream);
/* JointsOHKMMSELoss (core/loss.py:140-182), online hard key-point mining: per-joint loss
 *   l[n][k] = 0.5/HW * w[n][k]^2 * sum_hw (p-g)^2 ;  S_n = the topk joints of sample n with the largest l[n][.] ;
 *   loss = 1/(N*topk) * sum_n sum_{k in S_n} l[n][k] ;
 *   grad (NULL ok) = gscale * [k in S_n] * w^2 (p-g) / (HW*N*topk): exactly 0 for joints that were not selected.
 * Ties are broken towards the lower joint index (the loss does not depend on the rule, only the gradient does); a NaN
 * l ranks above every number, as in torch.topk, so exactly topk joints of every sample are selected.
 * pred/gt are [N][K][HW], w is [N][K] (NULL: weights 1).  1 <= topk <= K and K <= BUCTD_OHKM_MAX_JOINTS (one wavefront
 * ranks a sample) - anything else returns BUCTD_EINVAL.  workspace: buctd_joints_ohkm_mse_workspace(N, K) bytes (l and
 * the per-joint gradient scale).  Three launches (two without grad), no atomics: the result is deterministic. */
#define BUCTD_OHKM_MAX_JOINTS 64
size_t buctd_joints_ohkm_mse_workspace(int N, int K);
int buctd_joints_ohkm_mse(const float* pred, const float* gt, const float* w, int N, int K, int HW, int topk, float* loss,
                          float* grad, float gscale, void* workspace, size_t workspace_bytes, void* stream);
/* get_max_preds (core/inference.py:19-47): first-index argmax per [N*K] row of length H*W;
 * preds[row] = (x, y) zeroed where maxval <= 0. */
int buctd_argmax_decode(const float* hm, int rows, int H, int W, float* preds, float* maxvals, int32_t* idx,
                        void* stream);
/* the same plus the POST_PROCESS refinement of get_final_preds (core/inference.py:68-77): quarter[row] = the
 * (+-0.25 | 0, +-0.25 | 0) offset towards the higher neighbour for interior peaks, (0, 0) otherwise. */
int buctd_argmax_decode_refined(const float* hm, int rows, int H, int W, float* preds, float* maxvals, int32_t* idx,
                                float* quarter, void* stream);
/* get_final_preds(use_dark=True) (DarkPose, core/inference.py:90-151): preds / maxvals / idx exactly as
 * buctd_argmax_decode (from the unblurred map); offset[row] = the Taylor (Newton) step in heat-map pixels on
 * log(max(renormalised 11x11 Gaussian blur, 1e-10)) for peaks with 1 < px < W-2 and 1 < py < H-2, (0, 0) otherwise
 * or where the Hessian's determinant is 0.  POST_PROCESS does not apply.  H*W <= BUCTD_DARK_MAX_PIXELS (the float64
 * vertical pass sits in LDS); larger maps return BUCTD_EINVAL. */
#define BUCTD_DARK_MAX_PIXELS 8000
int buctd_argmax_decode_dark(const float* hm, int rows, int H, int W, float* preds, float* maxvals, int32_t* idx,
                             float* offset, void* stream);
/* generate_target (dataset/JointsDataset.py:397-453): joints [B][K][3] (crop px), vis [B][K] ->
 * target [B][K][Hh][Wh], weight [B][K]. */
int buctd_gaussian_target(const float* joints, const float* vis, int B, int K, int Hh, int Wh, float stride_x,
                          float stride_y, float sigma, float* target, float* weight, void* stream);
/* get_condition_image(_colored) (dataset/JointsDataset.py:500-543): joints [B][K][2+] (row stride js floats),
 * colors [K][Cc] (NULL: 255 mono) -> cond [B][Cc][H][W] in [0,255]; 15x15 Gaussian blur sigma 2.6 (reflect-101),
 * peak-normalised to 255 per image; truncate != 0 applies the mono path's .astype(int). workspace: B*Cc*H*W floats + B floats. */
size_t buctd_cond_render_workspace(int B, int Cc, int H, int W);
int buctd_cond_render(const float* joints, int js, const float* colors, int B, int K, int Cc, int H, int W,
                      int truncate, float* cond, void* workspace, size_t workspace_bytes, void* stream);
/* flip-test merge (core/function.py:226-236): out = 0.5*(a + shift(flip_back(b))) on [N][K][H][W];
 * perm[k] = source channel after the left/right swap; shift != 0 applies the 1-px SHIFT_HEATMAP. */
int buctd_flipback_avg(const float* a, const float* b, const int32_t* perm, int N, int K, int H, int W, int shift,
                       float* out, void* stream);

/* ------------------------------------------- gathered bf16x6 convolutions --- */
/* The convolutions around the BasicBlocks in the bf16x6 arithmetic (csrc/conv_gather_x6.hip): kind 1 = 1x1 / stride 1 /
 * pad 0 (fuse layers pose_hrnet.py:187-245, Bottlenecks :60-108), kind 2 = 3x3 / stride 2 / pad 1 (transitions :338-372,
 * fuse-layer downsampling), forward (dir 0) and data gradient (dir 1; a stride-2 data gradient runs its four output
 * parities as one launch).  (H, W) are the INPUT dims of the convolution, NHWC fp32 tensors, w is [Co][R][S][Ci];
 * Ci % 16 == 0, Co % 16 == 0, output channels of the launch a multiple of 48 or 64, H and W even for kind 2.
 * prep builds the weight image the kernels consume - once per weight update, per direction.  The forward takes the
 * epilogue options and Welford BatchNorm partials + counts of buctd_conv3x3_bf16x6 (groups from _stats_groups); the data
 * gradient adds `residual` (NULL ok) to dx.  Replace what cuDNN does for F.conv2d / its backward on those layers. */
int buctd_gconv_x6_supported(int kind, int N, int H, int W, int Ci, int Co, int dir);
size_t buctd_gconv_x6_prep_bytes(int kind, int Ci, int Co, int dir);
int buctd_gconv_x6_prep(int kind, int Ci, int Co, const float* w, int dir, void* wprep, void* stream);
/* all images of a model with ONE launch (after an optimizer step rewrote the filters in place): the caller fills one table
 * entry per (filter, direction) on the host with _prep_item (entry size _prep_item_bytes), uploads the table once, and
 * launches _prep_batched on it whenever the filters change. */
size_t buctd_gconv_x6_prep_item_bytes(void);
int buctd_gconv_x6_prep_item(int kind, int Ci, int Co, const float* w, int dir, void* wprep, void* item_host);
int buctd_gconv_x6_prep_batched(const void* items_device, int n, void* stream);
int buctd_gconv_x6_stats_groups(int kind, int N, int H, int W, int Ci, int Co, int* ngroups, int* rows_per_group);
int buctd_gconv_x6_fwd(int kind, int N, int H, int W, int Ci, int Co, const float* x, const void* wprep, const float* bias,
                       const float* scale, const float* shift, const float* residual, int relu, float* y,
                       float* stats_partials, int* stats_counts, void* stream);
/* forward with the output statistics added to an accumulator (buctd_bn_acc_bytes(Co), zero on entry) instead of partials */
int buctd_gconv_x6_fwd_acc(int kind, int N, int H, int W, int Ci, int Co, const float* x, const void* wprep, const float* bias,
                           float* y, void* stats_acc, void* stream);
int buctd_gconv_x6_dgrad(int kind, int N, int H, int W, int Ci, int Co, const float* dy, const void* wprep,
                         const float* residual, float* dx, void* stream);
/* Which kernel, tile plan and epilogue a launch of this shape takes (host code only, no launch; computed by the routing
 * function the launch itself goes through, so the answer cannot drift from it).  dir 0: _fwd / _fwd_acc, dir 1: _dgrad.
 * flags: which optional arguments the call would carry - 1 bias, 2 scale / shift, 4 relu, 8 partial-sum statistics,
 * 16 statistics accumulator (_fwd_acc: with the bias only), 32 residual (the only one a data gradient has).
 * out[25] = route (0 = gconv_x6_kernel, 1 = conv1x1_rows_x6_kernel), MF, NF, WM, WN, BM, BN, mode (-1 general epilogue,
 * 0 plain, 2 C3M_STATS, 4 C3M_RES of csrc/c3_lean.h), ncls, (ntaps, nhs, nsteps) of the four classes (0 beyond ncls), tiles,
 * ncol, and for route 1 - where everything between the route and here is 0 - NFT (16-column fragments) and the number of
 * K = 32 steps.  BUCTD_EINVAL: unsupported shape or flag set.  For tests that must know which code path a shape exercises. */
int buctd_gconv_x6_plan(int kind, int dir, int N, int H, int W, int Ci, int Co, int flags, int* out);
/* Weight gradient of a 1x1 (kind 1) or stride-2 3x3 pad-1 (kind 2; H, W even) convolution Ci -> Co in the bf16x6 arithmetic
 * (csrc/conv_gather_wgrad.hip): dw [Co][R][S][Ci] (+)= sum over output pixels dy (x) gathered x, x = [N][H][W][Ci], dy =
 * [N][Ho][Wo][Co].  The autograd weight gradient of the fuse-layer / transition / Bottleneck convolutions
 * (pose_hrnet.py:60-108, 187-245, 338-372); both channel counts must be multiples of 48, or both of 32. */
int buctd_gconv_wgrad_x6_supported(int kind, int N, int H, int W, int Ci, int Co);
/* the plan of that launch (no launch): out[8] = CF (64-, 48- or 32-channel chunk pairs: 4, 3, 2), TPG (taps per group), ntg
 * (tap groups), nsplit (K splits), q, rem (a split takes q k-steps of 32 output pixels, the first rem of them q + 1), ksteps,
 * and the pixels of a ragged last k-step (N * Ho * Wo % 32).  BUCTD_EINVAL: unsupported shape. */
int buctd_gconv_wgrad_x6_plan(int kind, int N, int H, int W, int Ci, int Co, int* out);
size_t buctd_gconv_wgrad_x6_workspace(int kind, int N, int H, int W, int Ci, int Co);
int buctd_gconv_wgrad_x6(int kind, int N, int H, int W, int Ci, int Co, const float* x, const float* dy, float* dw,
                         int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------- BasicBlock sequences --- */
/* The kernel sequences of residual BasicBlocks in train mode (pose_hrnet.py:28-57: stride 1, C -> C, no downsample, bf16x6
 * math) behind ONE call per direction, buctd_basic_chain_*: n chained blocks (an HRNet branch, pose_hrnet.py:165-185), n = 1
 * for a single block.  Per block: conv1 (+ statistics), conv2 with bn1 + ReLU applied in its input staging (+ statistics),
 * bn2 + skip + ReLU - three launches, the BatchNorm statistics travel as accumulators (no finalize) - and the mirrored
 * backward (two BatchNorm-backward applies, two data gradients that also form the BatchNorm sums, two weight gradients on
 * `side_stream`; NULL: same stream).  Pure launch sequences of the entry points above (bit-identical results); they exist
 * because a dozen calls per block through a Python binding cost more host time than HRNet-W32 needs GPU time.
 * The structs below describe ONE block.  acc: 2 * buctd_bn_acc_bytes(C) ZEROED bytes (forward statistics of conv1 | conv2);
 * stat: 4 * C floats receiving mean1, invstd1, mean2, invstd2 (saved for the backward).  running_* may be NULL. */
typedef struct {
  int N, H, W, C;
  const float* x;
  const void *w1_fwd, *w2_fwd;          /* prepared images, flip = 0 */
  const void *w1_bwd, *w2_bwd;          /* prepared images, flip = 1 (backward only) */
  const float *gamma1, *beta1, *gamma2, *beta2;
  float *running_mean1, *running_var1, *running_mean2, *running_var2;
  float eps1, momentum1, eps2, momentum2;
  float *z1, *z2, *y;
  void* acc;
  float* stat;
} buctd_basic_block;
typedef struct {
  const float* dy;                      /* gradient of the block output */
  float *dz2, *dres, *dy1, *dz1;        /* scratch tensors of the block's shape */
  float* dx;                            /* NULL: the block input needs no gradient */
  float *dw1, *dw2, *dgamma1, *dbeta1, *dgamma2, *dbeta2;
  int acc_w1, acc_w2, acc_bn1, acc_bn2; /* accumulate into (1) or overwrite (0) the gradient buffers */
  void* bn_acc;                         /* 2 * buctd_bn_acc_bytes(C) ZEROED bytes: backward sums of bn1 | bn2 */
  void* wg_ws; size_t wg_ws_bytes;      /* buctd_conv3x3_wgrad_bf16x6_workspace, used on `side_stream` */
} buctd_basic_block_grads;
/* blocks[k].x = blocks[k-1].y, grads[k].dy = grads[k+1].dx; the caller wires the pointers.  Inside a chain the sums of block
 * k-1's bn2 backward are formed by block k's conv1 data gradient. */
int buctd_basic_chain_fwd_train(int n, const buctd_basic_block* blocks, void* stream);
int buctd_basic_chain_bwd(int n, const buctd_basic_block* blocks, const buctd_basic_block_grads* grads, void* stream,
                          void* side_stream);

/* The branches of a HighResolutionModule (pose_hrnet.py:177-185, 247-249): nb independent chains of n blocks each, advanced
 * together - blocks[b * n + k] / grads[b * n + k] = block k of branch b, wired per branch as for buctd_basic_chain_*.  The
 * k-th convolutions of all branches are ONE launch (buctd_conv3x3_bf16x6_group), so are their BatchNorm applies, BatchNorm
 * backwards and weight gradients (buctd_conv3x3_wgrad_bf16x6_group on `side_stream`; each branch needs its own wg_ws of
 * buctd_conv3x3_wgrad_bf16x6_group_workspace(nb, ...) bytes): 3 launches per block step forward, 8 backward, whatever nb.
 * Activations, statistics and data gradients are bit-identical to nb buctd_basic_chain_* calls.  nb <= 4. */
int buctd_basic_branches_fwd_train(int nb, int n, const buctd_basic_block* blocks, void* stream);
int buctd_basic_branches_bwd(int nb, int n, const buctd_basic_block* blocks, const buctd_basic_block_grads* grads, void* stream,
                             void* side_stream);

/* Stream `to` waits for everything enqueued on stream `from` so far (one cached event per host thread and device): the fork in
 * front of work launched on a second stream, e.g. a weight gradient beside the data-gradient chain. */
int buctd_stream_fork(void* from, void* to);

/* ------------------------------------------------------------ bf16x6 GEMM --- */
/* C = alpha * A * B (+ bias) in the bf16x6 arithmetic of the 3x3 convolutions (fp32 operands split exactly into three
 * bf16 pieces, six bf16 MFMAs per product, fp32 accumulate) for the large plain GEMMs of the path - fc_o =
 * nn.Linear(T, T) of the CoAM channel attention (self_attention.py:150-159) forward, data and weight gradient.
 * Both operands are handed over as prepared images (fragment order, 6 bytes per element):
 *   image of a logical matrix X[v][k] (v: row of C for the A operand, column of C for the B operand; k: reduction
 *   index) whose element sits at src[(v / vg) * vgs + (v % vg) * vs + (k / kg) * kgs + (k % kg) * ks]
 *   (vg or kg = 0: no grouping, plain strides vs / ks).  role 0 = A operand, 1 = B operand (they differ in padding).
 * C(m, n) = C[m * ldc + (n / Nc) * gsc + n % Nc] (Nc <= 0: no grouping); bias_axis 0: bias[n], 1: bias[m]. */
int buctd_x6_image_dims(int V, int K, int role, int* Vpad, int* Kpad);
size_t buctd_x6_image_bytes(int V, int K, int role);
int buctd_x6_image(const float* src, int V, int K, int vg, long vgs, long vs, int kg, long kgs, long ks, int role,
                   void* image, void* stream);
int buctd_x6_gemm(int M, int N, int K, const void* a_image, const void* b_image, const float* bias, int bias_axis,
                  float alpha, float* C, long ldc, int Nc, long gsc, void* stream);
/* Host-only queries, no launch; each runs the code the launch itself runs.
 * buctd_x6_gemm_plan: what buctd_x6_gemm launches for M x N x K: out[8] = grid x (row tiles of 128), grid y (column tiles of
 *   192), row_major (1: consecutive workgroups of an XCD share the row tile), KB (32-slot steps of the padded K), chunks
 *   (KB / 2), total workgroups, total >> 3, total & 7.
 * buctd_x6_gemm_tile: the tile (bx, by) that the workgroup with linear id lin = blockIdx.y * gx + blockIdx.x computes on a
 *   gx x gy grid in the given order - the function the kernel calls.
 * buctd_x6_image_path: *vector = 1 where the lane of buctd_x6_image that holds row v, slots k0 .. k0 + 7 (k0 a multiple of
 *   8) reads them with two 16-byte loads, 0 where it gathers them one by one.  src is the pointer of the image call (the
 *   answer depends on its alignment); it is not dereferenced. */
int buctd_x6_gemm_plan(int M, int N, int K, int* out);
int buctd_x6_gemm_tile(int lin, int gx, int gy, int row_major, int* bx, int* by);
int buctd_x6_image_path(const float* src, int V, int K, int vg, long vgs, long vs, int kg, long kgs, long ks, int role,
                        int v, int k0, int* vector);

/* -------------------------------------------------------------- optimizer --- */
/* torch.optim.Adam step (utils/utils.py:268-272: betas .9/.999, eps 1e-8, no weight decay, no amsgrad)
 * on flat fp32 buffers; gscale multiplies the gradient first (1/world for averaged all-reduce). */
int buctd_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                    float eps, int step, float gscale, void* stream);
/* torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov) on a flat arena - the 'sgd' branch of get_optimizer
 * (lib/utils/utils.py:260-267).  first_step != 0: the momentum buffer is initialised with the gradient. */
int buctd_sgd_step(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum, float weight_decay,
                   int nesterov, int first_step, float gscale, void* stream);
/* The same steps with a clip coefficient that lives on the device: the gradient is multiplied by gscale * (*coef) before
 * anything else (SGD: before the weight-decay term, as torch clips p.grad before step() adds the decay).  coef is what
 * buctd_grad_clip_coef wrote; nothing is read back by the host.  *coef == 1.0f returns the bits of the plain steps (one
 * kernel body serves both forms). */
int buctd_adam_step_dscale(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                           float eps, int step, float gscale, const float* coef, void* stream);
int buctd_sgd_step_dscale(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                          float weight_decay, int nesterov, int first_step, float gscale, const float* coef, void* stream);

/* ------------------------------------------------------ parameter groups --- */
/* The same two steps over PARTS of the arena, each part with the hyper-parameters of its parameter group, as one launch
 * (engine.FusedAdam / FusedSGD with groups=: fine-tuning with a frozen trunk, a head at another learning rate, weight decay
 * on some tensors only).  The parts are given as a chunk table in device memory: chunk c is the len elements from element
 * start of p / g / m / v / buf and belongs to group `group` of the table passed by value.  Elements outside the chunks are
 * neither read nor written.  Workgroups walk the table with a grid stride; every access is 16 bytes wide, so start and len
 * are multiples of 4 (the arena pads every parameter to 16 bytes) and the buffers are 16-byte aligned.
 * Adam per element: coupled decay (decoupled == 0, torch.optim.Adam(weight_decay)) g = g * scale + weight_decay * p, then
 * the update of buctd_adam_step; decoupled (torch.optim.AdamW) p *= 1 - lr * weight_decay (formed in double by the host,
 * as torch forms it), then that update on the undecayed gradient.  With weight_decay == 0 both give the bits of
 * buctd_adam_step / _dscale on the same elements with the same hyper-parameters and step; the SGD form gives the bits of
 * buctd_sgd_step / _dscale with first_step = 0 (one set of per-element functions, csrc/step_math.h, serves all of them).
 * scale = gscale, times *coef where coef (device, what buctd_grad_clip_coef wrote) is not NULL. */
#define BUCTD_STEP_MAX_GROUPS 16
#define BUCTD_STEP_CHUNK 16384 /* elements, a multiple of 4 */
typedef struct {
  long start; /* first element; start % 4 == 0 */
  int len;    /* 0 < len <= BUCTD_STEP_CHUNK, len % 4 == 0 */
  int group;  /* 0 <= group < ngroups */
} buctd_step_chunk;
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  int decoupled;
  int step; /* this group's own step count, >= 1 in every group a chunk names (0: a group that has never stepped and is not
               named); the bias corrections are formed from it in double */
} buctd_adam_group;
typedef struct {
  float lr, momentum, weight_decay;
  int nesterov;
} buctd_sgd_group;
/* HOST only, no device call: cuts the nruns element runs [runs[2 r], runs[2 r + 1]) - run r owned by group run_group[r] -
 * into chunks of BUCTD_STEP_CHUNK elements counted from the run's first element (the last chunk of a run holds the rest)
 * and returns their number; out == NULL only counts.  Runs are given in ascending order.  Returns -1 (message in
 * buctd_last_error) for an empty, unaligned (start or end not a multiple of 4), descending or overlapping run and for a
 * group id outside [0, BUCTD_STEP_MAX_GROUPS). */
long buctd_step_chunks(const long* runs, const int* run_group, int nruns, buctd_step_chunk* out);
/* groups: HOST array of ngroups (1 .. BUCTD_STEP_MAX_GROUPS) entries, read during the call and handed to the kernel in its
 * arguments: nothing is copied to the device.  chunks_device: nchunks (> 0) entries as buctd_step_chunks wrote them; the
 * caller keeps every chunk inside the buffers and every group id below ngroups.  A group no chunk names costs nothing. */
int buctd_adam_step_groups(float* p, const float* g, float* m, float* v, const buctd_step_chunk* chunks_device, long nchunks,
                           const buctd_adam_group* groups, int ngroups, float gscale, const float* coef, void* stream);
/* buf: the momentum arena; may be NULL only where every group's momentum is 0 (it is not touched then) */
int buctd_sgd_step_groups(float* p, const float* g, float* buf, const buctd_step_chunk* chunks_device, long nchunks,
                          const buctd_sgd_group* groups, int ngroups, float gscale, const float* coef, void* stream);

/* ------------------------------------------------- gradient-norm clipping --- */
/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2, error_if_nonfinite False) on the flat gradient arena -
 * the reference clips between backward() and step() (lib/core/train.py:138-141).
 * buctd_grad_sumsq: *sumsq = sum of g[i]^2 over the nruns element runs [runs[2 r], runs[2 r + 1]) of g (runs: HOST array of
 * 2 nruns longs, 0 <= start < end; what FlatParams.grad_runs() returns).  Elements outside the runs are never read.  fp64
 * throughout (a float's square is exact there).  Order: every run is cut into chunks of BUCTD_GRAD_SUMSQ_CHUNK elements
 * counted from its first element, one partial sum per chunk in the workspace, added by one workgroup in a fixed order: the
 * result depends on the runs and the values alone, not on the grid or the number of CUs, and is bit-identical from launch to
 * launch (no floating-point atomics).  A run that starts on a 16-byte boundary is read with 16-byte loads and returns the
 * bits of the scalar path.  Workspace: 8 bytes per chunk, 8-byte aligned; buctd_grad_sumsq_workspace gives the size (0 for
 * a bad run list). */
#define BUCTD_GRAD_SUMSQ_CHUNK 8192
size_t buctd_grad_sumsq_workspace(const long* runs, int nruns);
int buctd_grad_sumsq(const float* g, const long* runs, int nruns, double* sumsq, void* workspace, size_t workspace_bytes,
                     void* stream);
/* total_norm = gscale * sqrt(*sumsq) ; coef = min(1, max_norm / (total_norm + 1e-6)) - torch's expressions, in fp64; both
 * are stored as one float each, on the device.  gscale: the scale the optimizer step applies to the gradient (1 / world),
 * so that the norm is the averaged gradient's.  A non-finite norm goes through the same expressions (inf -> coef 0,
 * NaN -> coef NaN): no special case. */
int buctd_grad_clip_coef(const double* sumsq, double gscale, double max_norm, float* coef, float* total_norm, void* stream);
/* abs_mean[s] = mean |g[i]|, norm[s] = sqrt(sum g[i]^2) over i in [spans[2 s], spans[2 s + 1]) for P segments (spans: DEVICE
 * array of 2 P longs - the parameters' spans in the arena): get_network_grad_flow (lib/utils/utils.py:293-300) without a
 * host trip per parameter.  fp64, one workgroup per segment, fixed order.  A monitor, not part of the step. */
int buctd_grad_segment_stats(const float* g, const long* spans, int P, double* abs_mean, double* norm, void* stream);

/* ------------------------------------------------------- weight averaging --- */
/* An averaged copy of the flat parameter arena (engine.WeightAverage: an exponential moving average, or SWA's equal
 * average), kept in a shadow buffer of the arena's layout (csrc/weight_avg.hip).  Per element
 *     avg[i] = fmaf(w, p[i] - avg[i], avg[i])
 * with w = 1 - decay for an EMA and 1 / (k + 1) for the k-th SWA sample, formed in double by the host and rounded once to
 * float.  The lerp form is the contract: p[i] == avg[i] and w == 0 leave avg[i] bit-unchanged (a zero keeps its sign too),
 * so frozen spans, constant tensors and the arena's zero padding need no table and one launch over the whole arena is right.
 * Any n >= 0 (0: no launch) and any alignment: 16-byte accesses when both pointers are 16-byte aligned (with a scalar tail of
 * n % 4 elements), a scalar kernel otherwise; both return the same bits.  Neither call allocates or synchronises.
 * BUCTD_EINVAL before any launch: n < 0, a NULL pointer with n > 0, p and avg ranges that overlap without being the same
 * buffer (p == avg is legal and changes nothing). */
int buctd_ema_update(const float* p, float* avg, long n, float w, void* stream);
/* The same rule over nitems separate tensors in ONE launch - the BatchNorm running statistics, which are module buffers
 * outside the arena.  items_device: a table in DEVICE memory (8-byte aligned), built once; workgroups walk it with a grid
 * stride.  An item may have any length (0 included: nothing happens) and alignment; the caller keeps every item inside its
 * buffers and the avg ranges of different items apart.  nitems == 0: no launch.  BUCTD_EINVAL: nitems < 0, a NULL or
 * misaligned table. */
typedef struct {
  const float* src;
  float* avg;
  long n;
} buctd_avg_item;
int buctd_ema_update_tensors(const buctd_avg_item* items_device, int nitems, float w, void* stream);
/* a[i] <-> b[i] for i in [0, n), one pass, no third buffer (the arena of the largest network is several hundred MB): puts
 * the averaged weights in front of the network and takes them out again.  Any n >= 0 and alignment, as above.
 * BUCTD_EINVAL before any launch: n < 0, a NULL pointer with n > 0, buffers that share a byte. */
int buctd_swap(float* a, float* b, long n, void* stream);

/* Fused self-attention (flash style, nothing T x T in memory) - nn.MultiheadAttention of the TransPose encoder layer
 * (transpose_h.py:168-213) and the CoAM attention cores (self_attention.py:74-86):
 *     out[b][i] = sum_j dropout(softmax_j(scale * q_i . k_j)) v_j   per head.
 * One calling form, the descriptor: h heads and q, k, v, out (dq, dk, dv) as separate tensors, each with its own row stride
 * in floats.  Head i reads columns [i dh, (i + 1) dh) of q, k, v and writes the same columns of out / dq / dk / dv; lse is
 * [B][h][T].  A packed one-head projection q | k is h = 1, k = q + dh, ldk = ldq.  Attention dropout draws the mask of
 * buctd_softmax_dropout_fwd on a [B][h][T][T] tensor: counter ((b h + head) T + query) T + key.
 * T % 64 == 0 (a last half block of query / key rows is masked), dh % 16 == 0, dh <= 128, Tq == Tk, dk == dv.
 * Every pointer 16-byte aligned, ldq / ldk / ldv / lddo multiples of 4.  Fields a pass does not use may be NULL / 0. */
typedef struct buctd_mha_args {
  int B, T, h, dh;
  const float* q; const float* k; const float* v;
  int ldq, ldk, ldv;
  float* out; int ldo;          /* forward: written; backward: the forward's result */
  float* lse;                   /* [B][h][T]; eval forward: NULL ok; train forward: written; backward: read */
  float scale, p_drop;          /* p_drop: train forward and backward only */
  const float* dout; int lddo;  /* backward */
  float* dq; float* dk; float* dv;
  int lddq, lddk, lddv;
} buctd_mha_args;
/* eval / no dropout.  buctd_mha_heads_fwd: exact fp32 MFMA.  _bf16x6: the bf16x6 arithmetic of the convolutions (three bf16
 * pieces per operand, six MFMAs per product, fp32 accumulate: fp32 class on the bf16 matrix cores); probabilities stay in
 * registers (S^T formulation). */
int buctd_mha_heads_fwd_supported(int T, int h, int dh);
int buctd_mha_heads_fwd(const buctd_mha_args* a, void* stream);
int buctd_mha_heads_fwd_bf16x6(const buctd_mha_args* a, void* stream);
/* bf16x6 attention over keys / values split ONCE per call into the workspace (6 B per element, the kernel's LDS tile layout)
 * and streamed into LDS by DMA: no per-workgroup re-split, K/V copies overlap the products, one image per XCD L2.  The same
 * pieces and products as buctd_mha_heads_fwd_bf16x6 with another association of the online soft-max (32-key tiles, the key
 * range in two halves that are merged): equal to fp32 round-off, not bit for bit.
 * Covers h == 1, T % 128 == 0, dh % 16 == 0, dh <= 128, ldo == dh, lse (NULL ok) [B][1][T]; ldk may differ from ldq.
 * buctd_mha_fwd_bf16x6_workspace(B, T, d): the bytes needed, 0 for a shape (T, d) this path does not cover. */
size_t buctd_mha_fwd_bf16x6_workspace(int B, int T, int d);
int buctd_mha_heads_fwd_bf16x6_ws(const buctd_mha_args* a, void* workspace, size_t workspace_bytes, void* stream);
/* TRAINING (autograd of softmax -> dropout -> . v), fused in both directions: forward with in-kernel attention dropout and
 * the row statistic lse; flash-style backward (one kernel template in two roles: dK/dV with the keys owned, dQ with the
 * queries owned).  Exact fp32 MFMA.  _dseed: the seed is read from device memory (a captured training step). */
int buctd_mha_heads_train_supported(int T, int h, int dh);
int buctd_mha_heads_fwd_train(const buctd_mha_args* a, uint64_t seed, void* stream);
size_t buctd_mha_heads_bwd_workspace(int B, int h, int T);              /* B h T floats: the row dots dout . out */
int buctd_mha_heads_bwd(const buctd_mha_args* a, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);
int buctd_mha_heads_fwd_train_dseed(const buctd_mha_args* a, const uint64_t* seed, void* stream);
int buctd_mha_heads_bwd_dseed(const buctd_mha_args* a, const uint64_t* seed, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Chosen rows of the attention matrix (the encoder's return_atten_map, transpose_h.py:110-150, 168-243), eval mode:
 *     out[b][r][j] = 1/h sum_head softmax_j(scale * q[rows[b][r]] . k[j])
 * straight from the projected q | k, nothing T x T unless every row is asked for.  Max-subtracted soft-max, products on
 * the exact fp32 MFMA in the contraction order of buctd_mha_heads_fwd, the head mean formed in head order by one lane per
 * element: two runs, duplicate rows, and a row query against the full map are bit-identical.
 * Any T >= 1, h >= 1, dh % 4 == 0, dh <= 128; q, k, out, out_heads 16-byte aligned, ldq / ldk multiples of 4 and >= h dh.
 * A row index outside [0, T) is no error: that row is written as exact zeros (an undetected joint). */
typedef struct buctd_attn_rows_args {
  int B, T, h, dh, R;               /* R query rows per image */
  const float* q; const float* k;   /* as buctd_mha_args: head i = columns [i dh, (i+1) dh) */
  int ldq, ldk;                     /* row strides in floats; images T*ld apart */
  const int* rows;                  /* device, [B][R] token index of each query row;
                                       NULL: R == T and row r is token r (the full map) */
  float scale;
  float* out;                       /* [B][R][T]  mean over heads of softmax_j(scale q_r . k_j) */
  float* out_heads;                 /* optional [B][h][R][T], NULL ok */
} buctd_attn_rows_args;
int buctd_attn_rows_supported(int T, int h, int dh);
int buctd_attn_rows(const buctd_attn_rows_args* a, void* stream);

/* ------------------------------------------------------- sample pipeline --- */
/* Person crop of the per-sample pipeline (dataset/JointsDataset.py:287-294): cv2.warpAffine(img_u8, M, (w, h),
 * flags=INTER_LINEAR) restated bit for bit (OpenCV's fixed-point bilinear, BORDER_CONSTANT 0), fused with
 * transforms.ToTensor + Normalize(mean, std); written into channels [0, 3) of the NCHW network input
 * (out + b * out_batch_stride).  flip: the source is mirrored horizontally first (JointsDataset.py:244);
 * rw > 0: source pixels outside the rectangle (rx, ry, rw, rh) read as zero (NEW_AUGMENTATION, 272-285).
 * crop_u8 (NULL ok): the 8-bit crop [B][h][w][3] (meta['input_img']).  items live in device memory. */
typedef struct {
  const unsigned char* src; /* uint8 [H][W][3], device memory */
  int H, W;
  int flip;
  int rx, ry, rw, rh;
  double m[6];              /* 2x3 forward matrix (source -> crop), as utils.transforms.get_affine_transform returns it */
} buctd_warp_item;
int buctd_warp_affine_norm(const buctd_warp_item* items_device, int B, int dst_h, int dst_w, const float* mean3,
                           const float* std3, float* out, long out_batch_stride, unsigned char* crop_u8, void* stream);
/* buctd_cond_render with a destination batch stride (in floats): renders straight into channels [3, 3+Cc) of the
 * network input. */
int buctd_cond_render_into(const float* joints, int js, const float* colors, int B, int K, int Cc, int H, int W,
                           int truncate, float* cond, long cond_batch_stride, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Condition key points of a generative-sampling train batch, from the synthesized poses to the render kernel's input
 * without leaving the device (JointsDataset.py:257-259 and 293-295, as DeviceSamplePipeline.geometry does them on the
 * host): per (sample, joint), with items[b].flip set, fliplr_joints - x = W - x - 1 (W = items[b].W), joints and
 * visibilities exchanged with pair[j] (-1: no partner), joints * visibilities - then (x, y) through items[b].m where
 * the (flipped) visibility's first column is > 0 (geom_point of sample.hip, which buctd_cond_mirror and
 * buctd_sample_geometry call as well).  synth (straight from buctd_synthesize_pose, image coordinates) and
 * cond_vis are float64 [B][K][3]; items_device is the table buctd_warp_affine_norm takes (only flip, W and m are read);
 * pair_device int [K].  out_joints / out_vis float64 [B][K][3]; out_trunc float32 [B][K][2] = trunc(x), trunc(y),
 * the `joints` argument of buctd_cond_render_into with js = 2.  float64 products and sums are never fused.  K <= 32. */
int buctd_cond_geometry(const double* synth, const double* cond_vis, const buctd_warp_item* items_device,
                        const int* pair_device, int B, int K, double* out_joints, double* out_vis, float* out_trunc,
                        void* stream);
/* The mirrored half of a flip-test input (reference lib/core/function.py:213-225), built on the device.
 * buctd_cond_mirror: the condition coordinates the mirrored crop is rendered from.  Per (sample, joint): fliplr_joints
 * (lib/utils/transforms.py:61-75) on crop coordinates - x' = (width - x) - 1 in float64, never fused; row and visibility
 * taken from pair[j] (-1: no partner); x' and y times the visibility's columns 0 and 1 (an invisible joint becomes
 * (0, 0)) - then trunc() toward zero and the conversion to float32 that buctd_cond_geometry and buctd_refine_step apply.
 * cond_joints float64 [B][K][joint_stride], joint_stride 2 (buctd_refine_args.cond_joints) or 3 - the coordinates BEFORE
 * truncation: trunc(width - 1 - x) is not width - 1 - trunc(x).  cond_vis float64 [B][K][3] or NULL = all ones.
 * out float32 [B][K][2], the `joints` argument of buctd_cond_render_into with js = 2.  K <= 32.
 * buctd_mirror_rows: out[b][channel0 + c][y][x] = in[b][channel0 + perm[c]][y][W - 1 - x] for c in [0, channels) over
 * float32 NCHW with dense images and batch strides in floats.  perm int32 [channels] on the device, an entry outside
 * [0, channels) keeps its channel (so the pair table with its -1 serves); NULL = identity.  in and out may be row ranges
 * of one tensor (rows [B, 2B) from rows [0, B)) but must not overlap.  Any W. */
int buctd_cond_mirror(const double* cond_joints, int joint_stride, const double* cond_vis, const int* pair_device, int B,
                      int K, int width, float* out, void* stream);
int buctd_mirror_rows(const float* in, long in_batch_stride, float* out, long out_batch_stride, const int32_t* perm,
                      int B, int channel0, int channels, int H, int W, void* stream);
/* One pass boundary of the iterative refinement (dataset.pipeline.IterativeRefiner; reference: three tools/test.py runs
 * chained through the results json, lib/dataset/dataloader.py:454-508 and 596-612): from the decode outputs of pass
 * `pass` to the crop affine and the condition of pass `pass` + 1 without leaving the device.  Per person, in the host's
 * order and with the host's roundings (float64 products and sums are never fused):
 *   preds      coords (+ offset) in float32 (core/inference.py DeferredFinalPreds.final_preds), through the inverse crop
 *              affine of (center, scale, heat-map size) in float64, rounded once to float32
 *              (utils.transforms.transform_preds(...).astype(float32));
 *   scores     keypoint_score = mean of the maxvals > float32(in_vis_thre), 0 when none is; score = keypoint_score *
 *              box_score, summed in float64 (IterativeRefiner.rescore);
 *   box        min / max of the non-zero x and of the non-zero y of the float32 preds, -+ margin, clipped to [0, W] and
 *              [0, H] with W, H = items[b].W, items[b].H (dataset.pipeline.box_from_keypoints: keypoint_box of sample.hip,
 *              shared with buctd_sample_geometry);
 *   center, scale   dataset.pipeline.xywh2cs (xywh2cs of sample.hip, shared likewise):
 *              float32(x + w * 0.5), float32(w / 200) * float32(scale_thre), the aspect branches and the
 *              center[0] != -1 test;
 *   items[b].m get_affine_transform(center, scale, 0, crop size) in the closed form of
 *              utils.transforms.crop_affine_closed_form; src, H, W, flip and the rectangle are not written;
 *   cond_trunc trunc() of the preds through the new m (all visibilities 1: IterativeRefiner.next_records), float32
 *              [B][K][2]: the `joints` argument of buctd_cond_render_into with js = 2.
 * center, scale (float32 [B][2]) and box_score (float64 [B]) are read as the values of this pass and overwritten with
 * those of the next.  Row `pass` of the history buffers receives this pass's preds (x, y, maxval), score, box_score,
 * keypoint_score, center and scale.  status (int32 [B], zeroed by the caller before the first pass, only ever or-ed
 * into): bit 0 - the person has no non-zero x or no non-zero y (the host raises ValueError from min() of an empty array),
 * bit 1 - the new box has no extent (the host's solve is singular); either way center, scale, m and cond_trunc of that
 * person stay as they are.  One wavefront per person, lanes over joints: K <= 32.  One launch, no allocation, no
 * synchronisation. */
typedef struct {
  const float* coords;      /* [B][K][2] heat-map coordinates of the decode kernels */
  const float* maxvals;     /* [B][K] */
  const float* offset;      /* [B][K][2] quarter-pixel or DARK offsets, NULL: none */
  float* center;            /* [B][2] in / out */
  float* scale;             /* [B][2] in / out */
  double* box_score;        /* [B] in / out */
  buctd_warp_item* items;   /* [B]: H, W read, m written */
  float* cond_trunc;        /* [B][K][2] out */
  double* cond_joints;      /* [B][K][2] out: the same coordinates before trunc(), NULL: not wanted */
  int32_t* status;          /* [B] */
  float* hist_preds;        /* [passes][B][K][3] */
  double* hist_score;       /* [passes][B] */
  double* hist_box_score;   /* [passes][B] */
  double* hist_keypoint_score; /* [passes][B] */
  float* hist_center;       /* [passes][B][2] */
  float* hist_scale;        /* [passes][B][2] */
  int B, K, pass, passes;
  int heatmap_w, heatmap_h, crop_w, crop_h;
  double margin, aspect_ratio, in_vis_thre, scale_thre;
} buctd_refine_args;
int buctd_refine_step(const buctd_refine_args* a, void* stream);
/* One frame boundary of CTD tracking (dataset.pipeline.SequenceTracker; reference call site: none: host loop - the
 * reference tracks by running its data loader once per frame).  M slots; the slot of a person is its identity, ids count
 * up from 0 and are never reused; the pose found in frame t is the condition of frame t + 1.  The call with `frame` = f
 * takes the decode outputs of frame f and leaves everything frame f + 1 needs, in this order:
 *   preds, score   of every live slot as buctd_refine_step forms them (box score 1); the float32 preds, widened, become
 *              the slot's pose.  An empty slot gets zeros.
 *   death      a live slot without a non-zero x or without a non-zero y among its preds, or whose box has no extent, dies
 *              at once; otherwise a keypoint score < death_score is one more miss (else misses = 0) and the slot dies at
 *              max_misses misses.
 *   merge      the survivors in ascending id order: a slot whose OKS against an older slot that is kept is >= merge_oks
 *              dies.  OKS: nms.oks_iou without a visibility threshold (nms_oks of csrc/oks.h, shared with
 *              buctd_oks_nms_grouped), areas = w * h of the pose boxes (box_from_keypoints with `margin`), fp64.
 *   birth      (f + 1 < frames) the detections [det_offsets[f + 1], det_offsets[f + 2]) by descending mean score (summed
 *              in joint order, / K), equal means by index: one whose OKS against every live slot - detections born before
 *              it in this call included - is < birth_oks takes the lowest free slot and the id *next_id, which counts up.
 *              Without a free slot it is dropped; so is one without a box.  The slots freed above are free here.
 *   next frame for every slot: center, scale (xywh2cs of the pose's box; an empty slot: of the whole image), items[s].m (the
 *              closed-form crop affine) and items[s].src = frame_src[f + 1]; cond_trunc = trunc() of the pose through m, zeros
 *              for an empty slot.  H, W, flip and the rectangle of an item are read, never written; all frames have the size
 *              of items[0].
 * History: row f receives preds, score and died; row f + 1 ids (-1: empty) and born.  `frame` = -1 is the birth of frame 0:
 * every slot must be empty (ids = -1) and coords / maxvals / offset are not read.  `frame` = frames - 1 ends with the merge.
 * Limits: M <= 64, K <= 32, max_dets <= 64 - the caller's statement of the largest detection count of a frame; detections
 * of a frame beyond it are never indexed.  One workgroup; the OKS tables (M x M, then M x D and the D x D triangle) are
 * built by all its lanes in LDS, the two greedy walks read LDS only; no atomics; deterministic.  One launch, no allocation,
 * no synchronisation. */
typedef struct {
  const float* coords;      /* [M][K][2] heat-map coordinates of the decode kernels, frame `frame` */
  const float* maxvals;     /* [M][K] */
  const float* offset;      /* [M][K][2] quarter-pixel or DARK offsets, NULL: none */
  int32_t* ids;             /* [M] in / out, -1: empty */
  int32_t* misses;          /* [M] in / out */
  int32_t* next_id;         /* [1] in / out */
  double* pose;             /* [M][K][3] in / out: x, y, score of every live slot */
  float* center;            /* [M][2] in / out */
  float* scale;             /* [M][2] in / out */
  buctd_warp_item* items;   /* [M]: H, W read; src, m written */
  float* cond_trunc;        /* [M][K][2] out */
  const double* dets;       /* [det_offsets[frames]][K][3]: x, y, score, image coordinates */
  const int32_t* det_offsets; /* [frames + 1] */
  const unsigned char* const* frame_src; /* [frames] device addresses of the frames, uint8 [H][W][3] */
  const double* sigmas;     /* [K] */
  int32_t* hist_ids;        /* [frames][M] */
  float* hist_preds;        /* [frames][M][K][3] */
  double* hist_score;       /* [frames][M] */
  unsigned char* hist_born; /* [frames][M] */
  unsigned char* hist_died; /* [frames][M] */
  int M, K, frame, frames, max_dets, max_misses;
  int heatmap_w, heatmap_h, crop_w, crop_h;
  double margin, aspect_ratio, in_vis_thre, scale_thre, birth_oks, merge_oks, death_score;
} buctd_track_args;
int buctd_track_step(const buctd_track_args* a, void* stream);
/* Scalar geometry of a TRAIN batch on the device (JointsDataset.py:217-295, as DeviceSamplePipeline.geometry restates
 * them on the host): from the records, the augmentation draws and (for generative sampling) the pose
 * buctd_synthesize_pose left on the device to the table buctd_warp_affine_norm reads and the inputs of
 * buctd_gaussian_target and buctd_cond_render_into.  Per sample, in the host's order and with the host's roundings
 * (float64 products and sums are never fused):
 *   box        flags & USE_BU_BBOX, a condition, its x sum != 0 and its joint 0 has y != 0: dataset.pipeline
 *              box_from_keypoints (non-zero coordinates -+ margin, clipped to [0, W] x [0, H] of items[b]) and xywh2cs
 *              with their float32 roundings; otherwise center / scale / bbox of the record.  (The x sum is a butterfly
 *              sum: it can differ from numpy's in the last bit, which matters only where the x cancel to rounding.)
 *   half body  flags & HALF_BODY: center, scale = half_body[b] (decided and boxed on the host);
 *   scale      float32 scale widened to float64, times draws[b][0] (numpy: float32 array * float64 scalar is float64);
 *   flip       flags & FLIP: center x = float32(float32(W - cx) - 1); fliplr_joints on the ground truth and the
 *              condition (x = W - x - 1, pair exchange, joints * joints_vis);
 *   m          get_affine_transform(center, scale, rot, crop size) in the closed form of
 *              utils.transforms.crop_affine_rot_closed_form with sin / cos = draws[b][1], draws[b][2];
 *   joints     ground truth and condition through m where vis[., 0] > 0; cond_trunc = trunc() of the condition;
 *              target_xy = dataset.pipeline.target_centres, target_vis = float32(vis[., 0]);
 *   rectangle  keep_rect set and the sample has a box (the record's, flags & HAS_BBOX, or the one formed above):
 *              x, y, w, h = trunc(bbox), with bbox_aug set widened by bbox_draws as JointsDataset.py:267-273 do, then
 *              cut at the origin (rx = max(x, 0), rw = x + w - rx: what oracle.sample.warp_affine_u8 keeps; the
 *              reference's negative slice indices wrap around instead - out of scope) into items[b].rx .. rh, zeros
 *              otherwise.  The kernel applies it to the mirrored image with the unmirrored box, like the reference.
 * status (int32 [B], written): bit 0 - USE_BU_BBOX and a condition without a non-zero x or without a non-zero y,
 * bit 1 - the box has no extent (the host's solve is singular); items[b] of such a sample stays as it is and its other
 * outputs are zeros.  One wavefront per sample, lanes over joints: K <= 32.  One launch, no allocation, no
 * synchronisation. */
#define BUCTD_GEOM_HAS_BBOX 1
#define BUCTD_GEOM_USE_BU_BBOX 2
#define BUCTD_GEOM_HALF_BODY 4
#define BUCTD_GEOM_FLIP 8
typedef struct {
  const double* joints;       /* [B][K][3] ground truth, image coordinates */
  const double* joints_vis;   /* [B][K][3] */
  const double* cond;         /* [B][K][3] condition pose, NULL (with cond_vis): non-conditional */
  const double* cond_vis;     /* [B][K][3] */
  const float* center;        /* [B][2] of the record */
  const float* scale;         /* [B][2] of the record */
  const double* bbox;         /* [B][4] x, y, w, h of the record (read with BUCTD_GEOM_HAS_BBOX) */
  const float* half_body;     /* [B][4] center, scale of the override (read with BUCTD_GEOM_HALF_BODY) */
  const double* draws;        /* [B][4] scale multiplier, sin, cos of the rotation, the rotation in degrees */
  const int32_t* bbox_draws;  /* [B][2] the two randint(0, 20) of BBOX_AUGMENTATION */
  const int32_t* flags;       /* [B] BUCTD_GEOM_* */
  const int32_t* pair;        /* [K] flip partner, -1: none */
  buctd_warp_item* items;     /* [B]: H, W read; flip, rx .. rh, m written */
  double* out_joints;         /* [B][K][3] crop coordinates */
  double* out_joints_vis;     /* [B][K][3] */
  double* out_cond;           /* [B][K][3], NULL with cond */
  double* out_cond_vis;       /* [B][K][3], NULL with cond */
  float* cond_trunc;          /* [B][K][2], NULL with cond */
  float* target_xy;           /* [B][K][3] the `joints` argument of buctd_gaussian_target */
  float* target_vis;          /* [B][K] */
  float* out_center;          /* [B][2] */
  double* out_scale;          /* [B][2] */
  double* out_rotation;       /* [B] */
  int32_t* status;            /* [B] */
  int B, K;
  int crop_w, crop_h;
  int keep_rect, bbox_aug;
  double margin, aspect_ratio, scale_thre;
  double stride_x, stride_y;  /* crop size / heat-map size */
} buctd_sample_geom_args;
int buctd_sample_geometry(const buctd_sample_geom_args* a, void* stream);

/* Generative pose synthesis(dataset/pose_synthesis.py:6-817, called from JointsDataset.py:202-215): for every person
 * and joint one of the error types jitter / miss / inversion / swap / good is drawn and a key point proposed
 * accordingly.  joints, estimated [B][K][3] and near_joints [B][M][K][3] (neighbours; visibility 0 = absent) are float64
 * device arrays, area [B] float64, num_overlap [B] int; out [B][K][3].  Randomness: a counter-based generator keyed by
 * (seed, person, joint) - pass a fresh seed per batch.  tables: per-dataset constants (host struct, copied). */
typedef struct {
  double sigmas[32];
  int pair[32];                /* symmetric partner of a joint, -1 = none (kps_symmetry) */
  int jitter_cls[32], miss_cls[32], inv_cls[32], swap_cls[32];
  double jitter_p[2][3];       /* [num_valid <= jitter_nv | else][class] */
  double miss_p[3][3];         /* [num_valid <= miss_nv[0] | <= miss_nv[1] | else][class] */
  double inv_p[3];
  double swap_p[2][3];         /* [crowded | else][class] */
  double out_vis;              /* third column of a synthesized joint: 1 (coco) / 0 (crowdpose, generic) */
  /* which row of a ladder a person takes (coco / crowdpose: 10; 5, 10; (10, 1), (15, 3) - the generic variant of every
   * other data set, synthesize_pose_fish: 4; 2, 4; (4, 1), (5, 1), no pair, all classes 0, sigmas 0.1) */
  int jitter_nv;               /* jitter_p row 0 while num_valid <= jitter_nv */
  int miss_nv[2];              /* miss_p row 0 while num_valid <= miss_nv[0], row 1 while <= miss_nv[1] */
  int crowd_nv[2], crowd_ov[2];/* crowded = (num_valid <= crowd_nv[i] and num_overlap >= crowd_ov[i]) for i = 0 or 1 */
} buctd_synth_tables;
int buctd_synthesize_pose(const buctd_synth_tables* tables, const double* joints, const double* estimated,
                          const double* near_joints, const double* area, const int* num_overlap, int B, int K, int M,
                          unsigned long long seed, double* out, void* stream);
/* Pose error diagnosis: the inverse of buctd_synthesize_pose.  Same inputs (`estimated` is the pose to diagnose, e.g. a
 * bottom-up model's), same limits (K <= 32, M <= 31).  With the synthesiser's sigmas, pairs, d85 / d50 rings (ks 0.85 and
 * 0.50 of sqrt(-2 area (2 sigma_j)^2 ln ks)) and sources, per person b and joint j - r0, rI, rS the float64 distances
 * sqrt(dx dx + dy dy) of estimated[j] to joints[j], to joints[pair[j]] (labelled) and to the nearest neighbours' joint j
 * or pair[j] (visibility > 0), +inf where there is none:
 *   code [B][K] int32   -1 joints[j] unlabelled (visibility <= 0) | 5 absent: estimated[j] is (0, 0) |
 *                       4 miss: min(r0, rI, rS) >= d50 | else the nearest source, ties own, inversion, swap:
 *                       r0 <= rI and r0 <= rS: 0 good (r0 < d85) or 1 jitter | rI <= rS: 2 inversion | 3 swap
 *   ks [B][K] float64   exp(-r0^2 / (2 area (2 sigma_j)^2)) where labelled and present, else 0
 *   hist [4][3][3][2] int64   type jitter / miss / inversion / swap x ladder row (the row buctd_synthesize_pose takes
 *                       for the person's num_valid and num_overlap; inversion: row 0) x the joint's class of that type x
 *                       {hits, eligible}.  Eligible: labelled and present - jitter and miss always, inversion where
 *                       its source exists, swap where a swap source exists.
 *   per_joint [K][6] int64   counts of the codes 0...5
 * hist and per_joint are ADDED to (64-bit integer atomics: the result does not depend on scheduling) - the caller
 * zeroes them, and may diagnose a data set in batches.  Classes outside [0, 3) and pairs >= K are refused. */
int buctd_pose_error_types(const buctd_synth_tables* tables, const double* joints, const double* estimated,
                           const double* near_joints, const double* area, const int* num_overlap, int B, int K, int M,
                           int* code, double* ks, long long* hist, long long* per_joint, void* stream);

/* ------------------------------------------------------------------- NMS --- */
/* Greedy box NMS - replaces _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
 * float nms_overlap_thresh, int device_id) of lib/nms/gpu_nms.hpp:1-2 / nms_kernel.cu:94-143 (kernel 33-77).
 * Differences of form, not of result: `boxes` ([boxes_num][boxes_dim], x1 y1 x2 y2 first, sorted by descending score
 * like gpu_nms.pyx:27-30 does before the call) is a DEVICE pointer, so are keep_out ([boxes_num] ints) and num_out;
 * the suppression mask lives in caller-provided workspace and the greedy sweep runs on the device as well.
 * A box is suppressed when IoU (with the +1 pixel convention) with an earlier kept box is > thresh. */
size_t buctd_nms_workspace(int boxes_num);
int buctd_nms(int* keep_out, int* num_out, const float* boxes, int boxes_num, int boxes_dim, float thresh,
              void* workspace, size_t workspace_bytes, void* stream);
/* cpu_nms(dets [n][5] float32, thresh) of lib/nms/cpu_nms.pyx:20-71 as plain host C++ (suppression at IoU >= thresh);
 * order = argsort of the scores, descending, computed by the caller like the .pyx does with numpy. */
int buctd_cpu_nms(const float* dets, int n, const int* order, float thresh, int* keep_out, int* num_out);

/* ------------------------------------------------------- keypoint evaluation --- */
/* The device part of core/keypoint_eval.py (csrc/keypoint_eval.hip): what the reference's data set classes do in
 * evaluate() with Python loops around lib/nms/nms.py and pycocotools.COCOeval (lib/dataset/dataloader.py:590-634,
 * 719-735).  All arithmetic is fp64.  Persons and ground truths are grouped by image with CSR offsets (int32
 * [images + 1]); the caller groups and, within an image, sorts persons by descending score (stable). */
/* Rescoring (dataloader.py:598-612): preds float32 [n][K][3] (x, y, joint score), box_in [n].  keypoint_score = mean of
 * the joint scores > in_vis_thre, added in joint order (0 if none); score = keypoint_score * box score; box_score is
 * the box score itself. */
int buctd_kpt_rescore(const float* preds, const double* box_in, int n, int K, double in_vis_thre, double* score,
                      double* box_score, double* keypoint_score, void* stream);
/* Greedy OKS suppression within every image (oks_nms / oks_iou of lib/nms/nms.py:75-124): one wavefront per image
 * walks its persons in the given (score) order; a kept person clears every later one whose OKS to it is > thresh.
 * OKS: variances (2 sigma)^2, scale = mean of the two areas + spacing(1); use_vis != 0 counts only the joints whose
 * score in the candidate is > in_vis_thre (OKS 0 if none).  kpts float32 [total][K][3], areas [total], sigmas [K];
 * keep int32 [total]: 1 kept, 0 suppressed.  max_per_image must be at least the largest group (it sizes the alive
 * bitmap in LDS, at most 524288); persons of a larger group beyond it are reported suppressed. */
int buctd_oks_nms_grouped(const int* offsets, int images, int max_per_image, const float* kpts, const double* areas,
                          const double* sigmas, int K, double thresh, int use_vis, double in_vis_thre, int* keep,
                          void* stream);
/* Soft OKS suppression within every image (soft_oks_nms / rescore of lib/nms/nms.py:150-200): one wavefront per image,
 * persons [offsets[i], offsets[i + 1]) in the caller's grouped order, n of them.  Every person's live score starts at
 * scores[p].  min(n, max_keep) rounds; in round r the head is the person not yet taken with the largest live score -
 * among equal live scores the lowest grouped position - and gets rank r; every other person not yet taken has its live
 * score multiplied by exp(-oks^2 / thresh) (decay_type 0, gaussian) or, decay_type 1 (linear), by 1 - oks where
 * oks >= thresh.  oks is the OKS of buctd_oks_nms_grouped against the head (use_vis / in_vis_thre look at the
 * candidate's joint scores).  This is the reference's re-sort per round written as an arg-max; the two agree whenever
 * no two live scores are equal.
 * kpts float32 [total][K][3], areas / scores [total], sigmas [K].  Outputs, both written for every person:
 * rank int32 [total] - the round in which the person was taken, -1 if it never was; soft_score [total] - the live score
 * the person had when it was taken, or after the last round if it was not.  soft_score holds the live scores during the
 * run, so n is unbounded; no LDS, no atomics.
 * BUCTD_EINVAL before any launch: a NULL pointer, images < 0, K <= 0, thresh <= 0, max_keep <= 0, decay_type not 0 / 1. */
int buctd_soft_oks_nms_grouped(const int* offsets, int images, const float* kpts, const double* areas,
                               const double* scores, const double* sigmas, int K, double thresh, int decay_type,
                               int use_vis, double in_vis_thre, int max_keep, double* soft_score, int* rank, void* stream);
/* OKS merge of prioritised prediction sets within every image (csrc/oks_merge.hip; oks_merge of lib/nms/nms.py:127-148
 * chained over the levels: merged = level 0; for l = 1 .. levels - 1: merged = oks_merge(level l, merged)).  One
 * wavefront per image.  The n persons are in grouped order, image-major and within an image level-major, level 0 the
 * highest priority; cells int32 [images * levels + 1] are the CSR offsets over the (image, level) cells: persons
 * [cells[i * levels + l], cells[i * levels + l + 1]) are level l of image i, cells[0] = 0, cells[images * levels] = n.
 * Every level-0 person is accepted.  A person of level l >= 1 is accepted iff the largest OKS between it and the
 * accepted persons of the levels < l of its image is <= thresh, or there is no such person.  Persons of one level are
 * not compared with each other, and a rejected person takes part in no later comparison.  The OKS is that of
 * buctd_oks_nms_grouped with the candidate as g and the accepted pose as d: use_vis / in_vis_thre look at the joint
 * scores of the accepted pose (nms.py:142 into nms.py:90-91).
 * kpts float32 [n][K][3], areas [n], sigmas [K].  Outputs, all written for every person: keep int32 [n] - 1 accepted,
 * 0 rejected; max_oks [n] - the largest OKS found, -1.0 for level 0 and where no accepted person precedes; best int32
 * [n] - the grouped index of the accepted person that gave max_oks, the lowest among equal values, -1 where max_oks is
 * -1.0.  A NaN OKS makes max_oks NaN (best: the first pose that gave one) and rejects the person, like numpy's max.
 * No workspace, no LDS, no atomics; persons per cell, levels and K are unbounded.
 * BUCTD_EINVAL before any launch: images < 0, levels <= 0, n < 0, K <= 0, images * levels >= 2^31 - 1, a NULL pointer.
 * images == 0 or n == 0: success, nothing is launched. */
int buctd_oks_merge_grouped(const int* cells, int images, int levels, int n, const float* kpts, const double* areas,
                            const double* sigmas, int K, double thresh, int use_vis, double in_vis_thre, int* keep,
                            double* max_oks, int* best, void* stream);
/* COCO keypoint matching, per image: (a) the D x G matrix of COCOeval.computeOks - variances (2 sigma)^2, denominator
 * gt area + spacing(1), the visible ground-truth joints where there are any, otherwise the distance to the doubled
 * box (x0 = bx - bw, x1 = bx + 2 bw, likewise y) - written row-major to oks + oks_offsets[image]; (b) the greedy
 * matchings of COCOeval.evaluateImg, one per (area range, threshold) pair, at most 64 pairs.
 * Detections: the image's kept persons in score order, already cut to the detection limit; dt_kpts float32
 * [dt_total][K][3].  Ground truths: gt_kpts [gt_total][K][3] (x, y, v), gt_area, gt_bbox [gt_total][4] (x, y, w, h),
 * gt_flags int32 (bit 0: iscrowd, bit 1: num_keypoints == 0; non-zero = ignored in every range).
 * thresholds [n_thr], area_ranges [n_area][2] (lo, hi: outside = area < lo or area > hi).
 * dt_matched / dt_ignored int32 [n_area][n_thr][dt_total]: dt_matched = 1 + the ground truth's row (0: unmatched);
 * dt_ignored = the matched ground truth's ignore flag, or, unmatched, whether the extent box of the detection's
 * key points (max x - min x)(max y - min y) lies outside the range.  The workspace holds the per-range ground-truth
 * order and the per-pair taken flags, so the number of ground truths of an image is unbounded. */
typedef struct {
  int images, K, n_thr, n_area;
  long dt_total, gt_total;
  const int* dt_offsets;
  const int* gt_offsets;
  const long* oks_offsets; /* [images + 1], oks_offsets[i + 1] - oks_offsets[i] = D_i * G_i */
  const float* dt_kpts;
  const double* gt_kpts;
  const double* gt_area;
  const double* gt_bbox;
  const int* gt_flags;
  const double* sigmas;
  const double* thresholds;
  const double* area_ranges;
  double* oks;
  int* dt_matched;
  int* dt_ignored;
} buctd_kpt_match_args;
size_t buctd_coco_kpt_match_workspace(long gt_total, int n_thr, int n_area);
int buctd_coco_kpt_match(const buctd_kpt_match_args* a, void* workspace, size_t workspace_bytes, void* stream);
/* Crowding of the ground truths (check_valid_annotations, lib/analysis/evaluation.py:132-178), one wavefront per image.
 * valid[g] = the largest of the 3K key point values is not 0, area > 0, and the box cut to the image
 * (x1 = max(0, x), x2 = min(width - 1, x1 + max(0, w - 1)), likewise y) has x2 >= x1 and y2 >= y1.
 * num_overlaps[g] = the number of other valid ground truths of the image whose IoU with g is > iou_thresh, -1 where g
 * is not valid; the IoU is compute_iou of lib/utils/utils.py:557-588 on the raw (x, y, w, h) boxes, operation by
 * operation (0 where the denominator is 0).  gt_bbox [gt_total][4], gt_kpts [gt_total][K][3], gt_area [gt_total],
 * image_wh [images][2] (width, height), all fp64; valid / num_overlaps int32 [gt_total]. */
int buctd_kpt_crowding(const int* gt_offsets, int images, long gt_total, int K, const double* gt_bbox,
                       const double* gt_kpts, const double* gt_area, const double* image_wh, double iou_thresh, int* valid,
                       int* num_overlaps, void* stream);
/* COCOeval accumulate + summarize for `segments` independent small evaluations, one wavefront each, one lane per
 * (area range, threshold) pair.  seg_offsets int32 [segments + 1] into the detection axis of dt_matched / dt_ignored
 * ([n_area][n_thr][dt_total] as buctd_coco_kpt_match writes them); a segment's detections are in descending score
 * order.  max_seg_len must be at least the longest segment and at most 64 (detections beyond it are not read).
 * npig int32 [segments][n_area]: non-ignored ground truths per area range; rec_thrs [n_rec], n_rec <= 128.
 * Per pair: rc = tp / npig, pr = tp / (fp + tp + spacing(1)), the precision envelope from the right, the precision at
 * the left searchsorted position of every recall threshold (0 past the end); -1 where npig == 0; recall 0 and
 * precision 0 for a segment without detections.  stats [segments][10]: the ten figures of COCOeval.summarize for key
 * points (AP, AP at thresholds t_half / t_three_q, AP of area ranges 1 and 2, the same five for AR), each the mean of
 * the entries > -1, added in index order, or -1 where none counts.  recall [segments][n_thr][n_area]. */
int buctd_kpt_segment_ap(const int* seg_offsets, int segments, int max_seg_len, long dt_total, const int* dt_matched,
                         const int* dt_ignored, int n_area, int n_thr, const int* npig, const double* rec_thrs, int n_rec,
                         int t_half, int t_three_q, double* stats, double* recall, void* stream);

/* ------------------------------------------------------- condition records --- */
/* The device part of dataset/conditions.py (csrc/conditions.hip): from a bottom-up model's poses to the records the
 * sample pipeline consumes - what the reference does with Python loops in data_preprocessing/match_coco_cond.py:79-103
 * and lib/dataset/dataloader.py:213-241, 335-393.  All arithmetic is fp64, operation by operation as the reference
 * states it, so the values equal the host's bit for bit; inputs are finite.  Groups (the poses / annotations of an
 * image) are CSR offsets, int32 [images + 1]; one wavefront takes one image and its lanes stride over the members, so
 * a group may have any size.  No function allocates or synchronises. */
#define BUCTD_POSE_BOX_ALL_POINTS 0
#define BUCTD_POSE_BOX_NONZERO 1
/* Boxes of n poses [n][K][3] (x, y, anything), one thread per pose.
 * BUCTD_POSE_BOX_ALL_POINTS (calc_bboxes_from_keypoints, match_coco_cond.py:19-30): min / max of x and of y over the
 *   joints with joint_mask[pose][joint] != 0 (int32 [n][K]; NULL: every joint), negative corners set to 0; boxes[pose]
 *   = x1, y1, x2, y2.  margin is not read.
 * BUCTD_POSE_BOX_NONZERO (dataloader.py:357-361): min / max of the x != 0 and, separately, of the y != 0; boxes[pose]
 *   = x, y, w, h = xmin - margin, ymin - margin, (xmax + margin) - (xmin - margin), likewise h.  joint_mask is not read.
 * status[pose] = 1 and a zero box where there is no x or no y to take a minimum over (the reference raises), else 0. */
int buctd_pose_boxes(const double* poses, int n, int K, int form, const int* joint_mask, double margin, double* boxes,
                     int* status, void* stream);
/* For every annotation the prediction of the same image with the largest _get_iou (match_coco_cond.py:33-50, on
 * x1 y1 x2 y2 boxes; ties go to the lowest row, and if every IoU is 0 that is the image's first prediction, as
 * np.argmax has it).  matched int32 [gt total]: the row of the prediction in pred_boxes, or -1 for an image without
 * predictions or an annotation with gt_status != 0 (gt_status may be NULL); best_iou [gt total]: its IoU, 0 with -1. */
int buctd_match_boxes(const int* gt_offsets, const int* pred_offsets, int images, const double* gt_boxes,
                      const int* gt_status, const double* pred_boxes, int* matched, double* best_iou, void* stream);
#define BUCTD_GROUP_IOU_TEST 0
#define BUCTD_GROUP_IOU_TRAIN 1
/* Per member of a group, over the x y w h boxes of the group:
 * BUCTD_GROUP_IOU_TEST (dataloader.py:368-372): max_iou = the largest JointsDataset.compute_iou with another member
 *   (0 where its denominator is 0), 0 for a single member; status 0; near_count is not written.
 * BUCTD_GROUP_IOU_TRAIN (dataloader.py:234-241): calc_bbox_overlap with every member, itself included; max_iou = the
 *   largest overlap that is != 1 in a group of more than one member (0 if none is left, where the reference raises),
 *   else 0; near_count[member] (may be NULL) = the number of overlaps > 0; a zero union (the reference divides by it)
 *   counts as overlap 0 and sets status[member] = 2. */
int buctd_group_max_iou(const int* offsets, int images, const double* boxes, int form, double* max_iou, int* status,
                        int* near_count, void* stream);
/* The near lists of the train form: near_offsets int64 [members + 1] is the prefix sum of near_count; member i's rows
 * (positions in `boxes`) of the members it overlaps by > 0 go to near_index[near_offsets[i] ...] in ascending order. */
int buctd_group_near_list(const int* offsets, int images, const double* boxes, const long* near_offsets,
                          int* near_index, void* stream);

/* ------------------------------------------------------------ debug pictures --- */
/* The pictures of utils/vis.py (csrc/vis.hip), rendered on the device into uint8 RGB; what the reference does with
 * cv2 / torchvision on fp32 host copies (utils/vis.py:75-141, 269-332).  The batch image is fp32 [B][3][H][W] given by
 * its four element strides sb, sc, sh, sw, so NCHW and channels-last tensors and views both work.  Every value is an
 * integer expression of bytes or the fp32 expression written here, one operation after the other (the library is built
 * without contraction).  No function allocates or synchronises; a null pointer (where none is allowed), an extent < 1
 * or an `out` that is not 4-byte aligned returns BUCTD_EINVAL before any launch.
 *
 * image byte of a value v: u = (v - lo) / ((hi - lo) + 1e-5f), then u * 255.0f clamped to [0, 255] and truncated; lo
 * and hi are read from lohi[0], lohi[1] in device memory.  lohi NULL: u = v (normalize=False).
 * bgr != 0: the image's channels are B, G, R (DATASET.COLOR_RGB false) and are swapped, so `out` is RGB either way. */
/* lohi[0] = the smallest, lohi[1] = the largest value of the image (finite values).  Two launches. */
int buctd_vis_minmax(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw, float* lohi,
                     void* stream);
/* save_batch_heatmaps: out uint8 [B*Hh][(K+1)*Wh][3].  Row block i is image i; column block 0 is the image shrunk to
 * Hh x Wh, column block j+1 is joint j.  heatmaps fp32 [B][K][Hh][Wh]; peaks fp32 [B][K][2] = (x, y) in heat-map
 * pixels, as the argmax decode writes them.
 *   shrunken image: bilinear, half-pixel centres, fixed-point weights, on the image bytes.  Per axis
 *     fx = (x + 0.5f) * ((float)W / (float)Wh) - 0.5f, x0 = floorf(fx), a = fx - x0; x0 < 0: x0 = 0, a = 0;
 *     x0 >= W - 1: x0 = W - 1, a = 0, the right tap is x0 itself; wa = (int)rintf(a * 2048.0f), likewise wb in y;
 *     byte = ((p00*(2048-wa) + p01*wa)*(2048-wb) + (p10*(2048-wa) + p11*wa)*wb + (1 << 21)) >> 22.
 *   heat byte: h * 255.0f clamped to [0, 255], truncated.  colour of a heat byte, on t = byte / 255.0f:
 *     r, g, b = clamp(1.5f - fabsf(4t - 3 | 2 | 1), 0, 1), each stored as (int)floorf(c * 255.0f + 0.5f).
 *   tile j+1 = (7 * colour + 3 * background) / 10 per channel in integers.
 *   marker of joint j: the four pixels at Manhattan distance 1 from ((int)px, (int)py), clipped to the tile, pure red.
 *     The markers are drawn onto the shrunken image joint after joint: the background of tile j+1 carries the markers
 *     of the joints 0..j (blended), joint j's own marker lies on top unblended, column block 0 carries all K. */
int buctd_vis_heatmap_grid(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw, const float* lohi,
                           const float* heatmaps, int K, int Hh, int Wh, const float* peaks, int bgr, uint8_t* out,
                           void* stream);
/* save_batch_image_with_joints: the make_grid picture of the batch, xmaps = min(nrow, B) cells per row, ymaps =
 * ceil(B / xmaps) rows, out uint8 [ymaps*(H+padding)+padding][xmaps*(W+padding)+padding][3]; image k sits at row
 * (k / xmaps)*(H+padding)+padding, column (k % xmaps)*(W+padding)+padding; padding and unused cells are 0, the rest
 * image bytes.  Marks per joint, in joint order, later ones painting over earlier ones, clipped to the cell's H x W:
 *   pred [B][K][2] where pred_vis [B][K] != 0: the disc dx*dx + dy*dy <= 8, red;
 *   gt where gt_vis != 0: a + with arms of 2 pixels, blue;
 *   cond where cond_vis > 0 and both coordinates > 0: an x with arms of 2 pixels, green (cond and cond_vis may both
 *   be NULL).  Positions are fp32 input pixels, truncated toward zero. */
int buctd_vis_joint_grid(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw, const float* lohi,
                         int K, const float* pred, const float* pred_vis, const float* gt, const float* gt_vis,
                         const float* cond, const float* cond_vis, int nrow, int padding, int bgr, uint8_t* out,
                         void* stream);

/* Pose overlays (csrc/vis_pose.hip): the skeletons of any number of persons drawn onto any number of uint8 RGB
 * canvases of different sizes, in place, in one launch - what the reference does with cv2.line / cv2.circle person after
 * person (tools/vis.py:plot_keypoints, lib/utils/vis.py:vis_keypoints).  Every table lies in device memory.
 *
 * Joint.  Joint j of person p is joints[(p*K + j)*3 ...] = x, y, score.  It counts only if x, y and score are finite
 * and score > score_thresh.  Its pixel is ((int)x + dx, (int)y + dy), truncation toward zero, (dx, dy) the person's
 * offset; a pixel coordinate outside [-8192, 8191] makes the joint absent.
 * End point.  A limb is (a0, a1, b0, b1, colour): end A is the floor midpoint of the pixels of the joints a0 and a1,
 * (xa0 + xa1) >> 1 and (ya0 + ya1) >> 1 with an arithmetic shift, valid if both joints count (a0 == a1: a plain joint);
 * end B likewise.  colour is a row of the palette or -1 for the person's colour.  A limb with a joint index outside
 * [0, K) or a colour outside [-1, n_palette) is not drawn.
 *
 * Coverage of pixel X, exact in 64-bit integers.  Coordinates lie in [-8192, 8191], so a difference is below 2^14, a
 * dot product below 2^29, and with thickness, radius <= 16384 every product below stays under 2^62.
 *   segment P-Q of thickness t: 4 d^2 <= t^2, d the distance from X to the segment.  v = Q - P, w = X - P, c1 = w.v,
 *     c2 = v.v;  c1 <= 0: 4 |w|^2 <= t^2;  c1 >= c2: 4 |X - Q|^2 <= t^2;  else 4 (|w|^2 c2 - c1^2) <= t^2 c2.
 *     P == Q is the first case.
 *   disc of radius r at Z: |X - Z|^2 <= r^2.
 *   ring of radius r and thickness t at Z: (2r - t)^2 <= 4 |X - Z|^2 <= (2r + t)^2, the lower bound dropped when 2r <= t.
 *
 * Paint order: persons in table order (canvas c owns the persons person_offsets[c] .. person_offsets[c+1] - 1), and
 * within a person
 *   BUCTD_VIS_POSE_PLAIN (plot_keypoints): a ring (radius, thickness) at every counting joint in joint order, then the
 *     segment of every limb whose two ends are valid, in table order; all in the person's colour.
 *   BUCTD_VIS_POSE_PRETTY (vis_keypoints): per limb in table order the segment if both ends are valid, then the disc
 *     (radius) at A if valid, then at B if valid, all three in the limb's colour.
 * The last primitive that covers a pixel decides its colour.  A primitive covers only pixels inside the person's clip
 * rectangle [x0, x1) x [y0, y1) (canvas pixels) and the canvas.
 * Blend of a covered pixel, per channel: (img * (256 - alpha256) + colour * alpha256 + 128) >> 8.  No other byte is
 * written: uncovered pixels, the bytes of a row beyond 3*W and a canvas without persons keep their bits, and alpha256 = 0
 * writes nothing.
 *
 * One workgroup draws one BUCTD_VIS_POSE_TILE_W x BUCTD_VIS_POSE_TILE_H tile; `tiles` lists them as (canvas, tile
 * column, tile row) and is filled by the caller from the canvas sizes it knows (a canvas needs no tile where nobody is
 * drawn; a tile listed twice is an error of the caller).  A workgroup examines its canvas's primitives
 * BUCTD_VIS_POSE_CHUNK at a time.  Entries of `tiles` and person ranges that point outside the tables, and canvases
 * larger than canvas_h_max x canvas_w_max or with row_stride < 3*W, draw nothing. */
#define BUCTD_VIS_POSE_PLAIN 0
#define BUCTD_VIS_POSE_PRETTY 1
#define BUCTD_VIS_POSE_TILE_W 64
#define BUCTD_VIS_POSE_TILE_H 16
#define BUCTD_VIS_POSE_CHUNK 256
typedef struct buctd_vis_canvas {
  uint8_t* base;     /* pixel (x, y), channel c at base[y*row_stride + 3*x + c] */
  long row_stride;   /* bytes, >= 3*W */
  int H, W;          /* 1 .. 8192 */
} buctd_vis_canvas;
typedef struct buctd_vis_pose_args {
  const buctd_vis_canvas* canvases;   /* [C] */
  const int* person_offsets;          /* [C+1], ascending, person_offsets[C] <= P */
  const int* persons;                 /* [P][7]: dx, dy, clip x0, y0, x1, y1, colour r | g << 8 | b << 16 */
  const float* joints;                /* [P][K][3] */
  const int* skeleton;                /* [L][5]: a0, a1, b0, b1, colour */
  const uint8_t* palette;             /* [n_palette][3] r, g, b; may be NULL with n_palette 0 */
  const int* tiles;                   /* [n_tiles][3]: canvas, tile column, tile row */
  int C, P, K, L, n_palette, n_tiles;
  int canvas_h_max, canvas_w_max;     /* the largest H and W of the canvas table, <= 8192 */
  int style, thickness, radius;       /* thickness 1 .. 16384, radius 0 .. 16384 */
  float score_thresh;
  int alpha256;                       /* 0 .. 256 */
} buctd_vis_pose_args;
/* One launch, none when P or n_tiles is 0.  BUCTD_EINVAL before any launch: a NULL table, C < 1, P < 0, n_tiles < 0,
 * K or L outside 1 .. 64, n_palette < 0, an unknown style, thickness, radius, alpha256 or canvas_*_max out of range. */
int buctd_vis_pose_overlay(const buctd_vis_pose_args* a, void* stream);

/* ------------------------------------------------------------- bf16 inference --- */
/* Eval forward of the HRNet / preNet networks in bf16 storage (csrc/conv_bf16.hip, buctd_amd/ops_bf16.py).
 * bf16 tensors are passed as raw bit patterns (uint16_t).  Activations bf16 NHWC [N][H][W][C]; a conv layer is a
 * filter image wimg [Co][Kp] bf16, K = (r * R + s) * Ci + ci, zero-padded from R*R*Ci up to Kp = roundup(R*R*Ci, 32),
 * plus an fp32 bias [Co]; both come from buctd_bf16_pack_conv.  One bf16 MFMA per product, fp32 accumulation. */
/* wimg/bias_out = the conv (fp32 weight element (co, ci, r, s) at w[co*s_co + ci*s_ci + r*s_r + s*s_s], optional
 * conv_bias) with an optional eval BatchNorm folded in: scale = gamma / sqrt(var + eps) evaluated in fp64 and rounded
 * to fp32, then in fp32 w * scale rounded once to bf16 (nearest even) and bias (conv_bias - mean) * scale + beta.
 * gamma NULL: no BatchNorm. */
int buctd_bf16_pack_conv(const float* w, long s_co, long s_ci, long s_r, long s_s, int Co, int Ci, int R,
                         const float* conv_bias, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, uint16_t* wimg, float* bias_out, void* stream);
/* y = relu?(conv(x, wimg) + bias (+ residual)); R in {1, 3}, stride in {1, 2}, Ho = (H + 2 pad - R) / stride + 1.
 * out_f32_nchw = 0: y is bf16 NHWC [N][Ho][Wo][Co] and residual (optional) bf16 of the same shape;
 * out_f32_nchw = 1: y is fp32 NCHW [N][Co][Ho][Wo] (the heat-map head), no residual.  The kernels need no workspace
 * (workspace may be NULL). */
int buctd_bf16_conv(const uint16_t* x, int N, int H, int W, int Ci, const uint16_t* wimg, const float* bias, int Co,
                    int R, int stride, int pad, const uint16_t* residual, int relu, int out_f32_nchw, void* y,
                    void* workspace, size_t workspace_bytes, void* stream);
/* HighResolutionModule fuse row in bf16: out = relu(sum_j upsample_nearest(term_j, 2^shift_j)), terms read as bf16
 * and summed in fp32 in the order j = 0, 1, ..., rounded once; terms[j] is [N][H>>shift_j][W>>shift_j][C], C % 8 == 0,
 * up to 4 terms. */
int buctd_bf16_fuse_sum(const uint16_t* const* terms, const int* shifts, int nterms, int N, int H, int W, int C,
                        int relu, uint16_t* out, void* stream);
/* y = bf16(x), nearest even, n elements */
int buctd_bf16_from_f32(const float* x, long n, uint16_t* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
