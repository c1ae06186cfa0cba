// Native launch sequences of residual BasicBlocks in train mode (reference lib/models/pose_hrnet.py:28-57, stride 1,
// no downsample, bf16x6 math):  y = relu(bn2(conv2(relu(bn1(conv1(x))))) + x).
// Nothing is computed here: these entry points enqueue the kernels that the host mirror used to enqueue one ctypes call
// at a time (nine calls and a dozen small allocations per block and direction - ~95 us of Python per block forward,
// which made HRNet-W32 at 256x192 host-bound).  Same kernels, same order, same streams: results are bit-identical.
// ONE sequence (row_fwd_train / row_bwd: block k of every chain of a row of nb chains) fills the item structs of the group
// entry points; it is issued in one of two ways: the branches of a module (buctd_basic_branches_*) hand a row of items to a
// _group launch, a chain (buctd_basic_chain_*) is a row of one whose item is unpacked into the single-launch call.
#include "common.h"
#include "../../include/buctd_hip.h"
#include <string.h>

#define BLK_TRY(call)      \
  do {                     \
    const int rc_ = (call); \
    if (rc_) return rc_;   \
  } while (0)

static bool fwd_ptrs_ok(const buctd_basic_block& b) {
  return b.x && b.w1_fwd && b.w2_fwd && b.z1 && b.z2 && b.y && b.acc && b.stat;
}

static bool bwd_ptrs_ok(const buctd_basic_block& b, const buctd_basic_block_grads& g) {
  return b.x && b.w1_bwd && b.w2_bwd && b.z1 && b.z2 && b.y && b.stat && g.dy && g.dres && g.dy1 && g.dw1 && g.dw2 && g.bn_acc &&
         g.wg_ws && g.dz2 && g.dz1;
}


// Where a block keeps its BatchNorm statistics: stat = mean1 | invstd1 | mean2 | invstd2 ([C] floats each, written by the
// forward) and - forward (b.acc) and backward (g.bn_acc) alike - two accumulators, bn1's | bn2's (bn_acc.h; zero on entry).
static float* mean1_of(const buctd_basic_block& b) { return b.stat; }
static float* invstd1_of(const buctd_basic_block& b) { return b.stat + b.C; }
static float* mean2_of(const buctd_basic_block& b) { return b.stat + 2 * b.C; }
static float* invstd2_of(const buctd_basic_block& b) { return b.stat + 3 * b.C; }
static void* acc1_of(void* acc) { return acc; }
static void* acc2_of(void* acc, int C) { return (char*)acc + buctd_bn_acc_bytes(C); }

// the forward statistics of bn1 (second = 0) or bn2 (1) as the accumulator their consumer decodes
static void acc_in_of(const buctd_basic_block& b, int second, buctd_bn_acc_in* st) {
  st->acc = second ? acc2_of(b.acc, b.C) : acc1_of(b.acc);
  st->rows = (long)b.N * b.H * b.W;
  st->eps = second ? b.eps2 : b.eps1;
  st->momentum = second ? b.momentum2 : b.momentum1;
  st->mean_out = second ? mean2_of(b) : mean1_of(b);
  st->invstd_out = second ? invstd2_of(b) : invstd1_of(b);
  st->running_mean = second ? b.running_mean2 : b.running_mean1;
  st->running_var = second ? b.running_var2 : b.running_var1;
}

// the shape of a block's two C -> C convolutions; every pointer of the item is left NULL
static buctd_c3_conv c3_of(const buctd_basic_block& b) {
  buctd_c3_conv c;
  memset(&c, 0, sizeof(c));
  c.N = b.N; c.H = b.H; c.W = b.W; c.Ci = c.Co = b.C;
  return c;
}

// `to` waits for everything enqueued on `from` so far: event record + stream wait through one cached event per host thread
// AND device (an event belongs to the device it was created on).  `who` names the entry point in the error text.
static int stream_fork(hipStream_t from, hipStream_t to, const char* who) {
  if (from == to) return BUCTD_OK;
  static thread_local hipEvent_t evs[16] = {nullptr};
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= 16) {
    buctd_set_error("%s: cannot identify the current device", who);
    return BUCTD_ELAUNCH;
  }
  hipEvent_t& ev = evs[devid];
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    buctd_set_error("%s: hipEventCreate failed", who);
    return BUCTD_ELAUNCH;
  }
  if (hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess) {
    buctd_set_error("%s: stream fork failed", who);
    return BUCTD_ELAUNCH;
  }
  return BUCTD_OK;
}

// ---- issuing a row of items ------------------------------------------------------------------------------------------------
// group: the n items are ONE launch of the _group entry point.  Otherwise the row is one item, unpacked into the
// single-launch call (a chain never takes the group kernels: their weight-gradient split is not bit-identical to it).
static int issue_conv_fwd(bool group, int n, const buctd_c3_conv* c, void* s) {
  if (group) return buctd_conv3x3_bf16x6_group(n, c, s);
  return buctd_conv3x3_bf16x6_acc(c->N, c->H, c->W, c->Ci, c->Co, c->x, c->wprep, c->residual, c->relu, c->y, c->stats_acc,
                                  c->in_bn, c->in_gamma, c->in_beta, c->in_relu, s);
}
static int issue_dgrad(bool group, int n, const buctd_c3_conv* c, void* s) {
  if (group) return buctd_conv3x3_bf16x6_group(n, c, s);
  if (c->bn_acc)
    return buctd_conv3x3_bf16x6_bnstat_acc(c->N, c->H, c->W, c->Ci, c->Co, c->x, c->wprep, c->residual, c->y, c->bn_z, c->bn_y,
                                           c->bn_mean, c->bn_invstd, c->bn_gamma, c->bn_beta, c->bn_acc, s);
  return buctd_conv3x3_bf16x6(c->N, c->H, c->W, c->Ci, c->Co, c->x, c->wprep, nullptr, nullptr, nullptr, c->residual, 0, c->y,
                              nullptr, nullptr, s);
}
static int issue_wgrad(bool group, int n, const buctd_wg3_conv* c, void* s) {
  if (group) return buctd_conv3x3_wgrad_bf16x6_group(n, c, s);
  if (c->x_mean)
    return buctd_conv3x3_wgrad_bf16x6_bnin(c->N, c->H, c->W, c->Ci, c->Co, c->x, c->dy, c->dw, c->accumulate, c->x_mean,
                                           c->x_invstd, c->x_gamma, c->x_beta, c->x_relu, c->workspace, c->workspace_bytes, s);
  return buctd_conv3x3_wgrad_bf16x6(c->N, c->H, c->W, c->Ci, c->Co, c->x, c->dy, c->dw, c->accumulate, c->workspace,
                                    c->workspace_bytes, s);
}
static int issue_bn_apply(bool group, int n, const buctd_bn_apply_item* a, void* s) {
  if (group) return buctd_bn_apply_acc_group(n, a, s);
  return buctd_bn_apply_acc(a->z, &a->st, a->gamma, a->beta, a->residual, a->relu, a->y, a->rows, a->C, s);
}
static int issue_bn_bwd(bool group, int n, const buctd_bn_bwd_item* i, void* s) {
  if (group) return buctd_bn_bwd_acc_group(n, i, s);
  return buctd_bn_bwd_acc(i->dy, i->y, i->z, i->mean, i->invstd, i->gamma, i->beta, i->relu, i->rows, i->C, i->dz, i->dres,
                          i->dgamma, i->dbeta, i->accumulate, i->acc, i->acc_ready, s);
}

// ---- the sequence ----------------------------------------------------------------------------------------------------------
// A row of nb independent chains of n BasicBlocks each (blocks[b * n + k] = block k of chain b; block k's input is block
// k-1's output, in the backward its upstream gradient is block k+1's input gradient), advanced TOGETHER: per block step 3
// launches forward and 8 backward, whatever nb.  group = false needs nb = 1.
#define BR_MAX 4

static int row_fwd_train(bool group, int nb, int n, const buctd_basic_block* blocks, void* stream) {
  for (int k = 0; k < n; ++k) {
    buctd_c3_conv cv[BR_MAX];
    buctd_bn_acc_in st1[BR_MAX];
    buctd_bn_apply_item ap[BR_MAX];
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      buctd_c3_conv& c = cv[b] = c3_of(B);
      c.x = B.x; c.wprep = B.w1_fwd; c.y = B.z1; c.stats_acc = acc1_of(B.acc);
    }
    BLK_TRY(issue_conv_fwd(group, nb, cv, stream));
    // conv2 decodes bn1's statistics from its accumulator in its prologue (its first tile leaves mean1 / invstd1 for the backward
    // pass and updates the running statistics) and applies bn1 + ReLU while it stages its input: no finalize launch, and
    // relu(bn1(z1)) never exists in memory
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      buctd_c3_conv& c = cv[b];
      acc_in_of(B, 0, &st1[b]);
      c.x = B.z1; c.wprep = B.w2_fwd; c.y = B.z2; c.stats_acc = acc2_of(B.acc, B.C);
      c.in_bn = &st1[b]; c.in_gamma = B.gamma1; c.in_beta = B.beta1; c.in_relu = 1;
    }
    BLK_TRY(issue_conv_fwd(group, nb, cv, stream));
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      buctd_bn_apply_item& a = ap[b];
      a.z = B.z2;
      acc_in_of(B, 1, &a.st);
      a.gamma = B.gamma2; a.beta = B.beta2; a.residual = B.x; a.relu = 1; a.y = B.y;
      a.rows = a.st.rows; a.C = B.C;
    }
    BLK_TRY(issue_bn_apply(group, nb, ap, stream));
  }
  return BUCTD_OK;
}

// b, g: element k > 0 of a chain's arrays.  Block k - 1 can take its bn2 sums from block k's conv1 data gradient if that
// gradient IS its upstream gradient, the two blocks have one shape and share the workspace the sums travel in
static bool bn2_sums_chain(const buctd_basic_block* b, const buctd_basic_block_grads* g) {
  return g->dx && g->dx == g[-1].dy && g[-1].bn_acc && b[-1].y == b->x && b[-1].N == b->N && b[-1].H == b->H && b[-1].W == b->W &&
         b[-1].C == b->C;
}

// The sums of each BatchNorm backward (sum g, sum g zhat over the batch) are a by-product of the data gradient that PRODUCES g
// (its epilogue has the tile in registers): bn1's of conv2's data gradient, bn2's - inside a chain - of the conv1 data
// gradient of the block behind.  They travel as integer accumulators (g.bn_acc).  The weight gradients run on the side
// stream behind the kernel that produced their dY operand.  `who` names the entry point in error texts.
static int row_bwd(bool group, const char* who, int nb, int n, const buctd_basic_block* blocks,
                   const buctd_basic_block_grads* grads, void* stream, void* side_stream) {
  hipStream_t main_s = (hipStream_t)stream, side_s = side_stream ? (hipStream_t)side_stream : main_s;
  bool ready[BR_MAX] = {false, false, false, false};     // block k's bn2 sums were formed by block k + 1's conv1 data gradient
  for (int k = n - 1; k >= 0; --k) {
    buctd_bn_bwd_item bi[BR_MAX];
    buctd_wg3_conv wg[BR_MAX];
    buctd_c3_conv cv[BR_MAX];
    bool chain[BR_MAX];      // this step's conv1 data gradient forms the bn2 sums of the block in front
    // conv2 / bn2 (+ skip): dres = masked upstream gradient
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      chain[b] = k > 0 && bn2_sums_chain(&B, &G);
      bi[b] = buctd_bn_bwd_item{G.dy, B.y, B.z2, mean2_of(B), invstd2_of(B), B.gamma2, nullptr, 1, (long)B.N * B.H * B.W, B.C,
                                G.dz2, G.dres, G.dgamma2, G.dbeta2, G.acc_bn2, acc2_of(G.bn_acc, B.C), ready[b] ? 1 : 0};
    }
    BLK_TRY(issue_bn_bwd(group, nb, bi, stream));
    BLK_TRY(stream_fork(main_s, side_s, who));
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      wg[b] = buctd_wg3_conv{B.N, B.H, B.W, B.C, B.C, B.z1, G.dz2, G.dw2, G.acc_w2, mean1_of(B), invstd1_of(B), B.gamma1, B.beta1,
                             1, G.wg_ws, G.wg_ws_bytes};
    }
    BLK_TRY(issue_wgrad(group, nb, wg, side_s));
    // conv2's data gradients dy1, and with them the sums of bn1's backward (ReLU mask rebuilt from z1)
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      buctd_c3_conv& c = cv[b] = c3_of(B);
      c.x = G.dz2; c.wprep = B.w2_bwd; c.y = G.dy1;
      c.bn_z = B.z1; c.bn_mean = mean1_of(B); c.bn_invstd = invstd1_of(B); c.bn_gamma = B.gamma1; c.bn_beta = B.beta1;
      c.bn_acc = acc1_of(G.bn_acc);
    }
    BLK_TRY(issue_dgrad(group, nb, cv, stream));
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      bi[b] = buctd_bn_bwd_item{G.dy1, nullptr, B.z1, mean1_of(B), invstd1_of(B), B.gamma1, B.beta1, 1, (long)B.N * B.H * B.W, B.C,
                                G.dz1, nullptr, G.dgamma1, G.dbeta1, G.acc_bn1, acc1_of(G.bn_acc), 1};
    }
    BLK_TRY(issue_bn_bwd(group, nb, bi, stream));
    BLK_TRY(stream_fork(main_s, side_s, who));
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      wg[b] = buctd_wg3_conv{B.N, B.H, B.W, B.C, B.C, B.x, G.dz1, G.dw1, G.acc_w1, nullptr, nullptr, nullptr, nullptr, 0,
                             G.wg_ws, G.wg_ws_bytes};
    }
    BLK_TRY(issue_wgrad(group, nb, wg, side_s));
    // conv1's data gradients, of the chains that want dx only (the row is compacted); the skip gradient joins in the epilogue;
    // inside a chain the output is the upstream gradient of the block in front, whose bn2 sums are formed on the way out
    int m = 0;
    for (int b = 0; b < nb; ++b) {
      const buctd_basic_block& B = blocks[b * n + k];
      const buctd_basic_block_grads& G = grads[b * n + k];
      ready[b] = chain[b];
      if (!G.dx) continue;
      buctd_c3_conv& c = cv[m++] = c3_of(B);
      c.x = G.dz1; c.wprep = B.w1_bwd; c.residual = G.dres; c.y = G.dx;
      if (chain[b]) {
        const buctd_basic_block& Bp = blocks[b * n + k - 1];
        c.bn_z = Bp.z2; c.bn_y = Bp.y; c.bn_mean = mean2_of(Bp); c.bn_invstd = invstd2_of(Bp); c.bn_gamma = Bp.gamma2;
        c.bn_acc = acc2_of(grads[b * n + k - 1].bn_acc, B.C);
      }
    }
    if (m) BLK_TRY(issue_dgrad(group, m, cv, stream));
  }
  return BUCTD_OK;
}

// A residual CHAIN (the four BasicBlocks of an HRNet branch, pose_hrnet.py:165-185 _make_one_branch; n = 1: one block): a row
// of one, every item through its single-launch entry point, behind ONE call per direction.  What it saves is host time - the
// HRNet-W32 step is bound by it, and the W48 step starves the GPU wherever the maps are small.
extern "C" int buctd_basic_chain_fwd_train(int n, const buctd_basic_block* blocks, void* stream) {
  BUCTD_CHECK_ARG(n > 0 && blocks, "buctd_basic_chain_fwd_train: bad argument");
  for (int k = 0; k < n; ++k) BUCTD_CHECK_ARG(fwd_ptrs_ok(blocks[k]), "buctd_basic_chain_fwd_train: null pointer in block %d", k);
  return row_fwd_train(false, 1, n, blocks, stream);
}
extern "C" int buctd_basic_chain_bwd(int n, const buctd_basic_block* blocks, const buctd_basic_block_grads* grads, void* stream,
                                     void* side_stream) {
  BUCTD_CHECK_ARG(n > 0 && blocks && grads, "buctd_basic_chain_bwd: bad argument");
  for (int k = 0; k < n; ++k)
    BUCTD_CHECK_ARG(bwd_ptrs_ok(blocks[k], grads[k]), "buctd_basic_chain_bwd: null pointer in block %d", k);
  return row_bwd(false, "buctd_basic_chain_bwd", 1, n, blocks, grads, stream, side_stream);
}

// The branches of a HighResolutionModule (pose_hrnet.py:177-185, 247-249): the k-th convolutions of all branches are one
// launch (buctd_conv3x3_bf16x6_group: their tiles form one grid of several de-phased rounds instead of nb phase-locked single
// rounds on nb streams), and so are the BatchNorm applies, the BatchNorm backwards and the weight gradients.  Forward and
// data gradients are bit-identical to the per-branch chains; the weight gradients use the group split
// (buctd_conv3x3_wgrad_bf16x6_group: fixed order, fp32-class).
extern "C" int buctd_basic_branches_fwd_train(int nb, int n, const buctd_basic_block* blocks, void* stream) {
  BUCTD_CHECK_ARG(nb > 0 && nb <= BR_MAX && n > 0 && blocks, "buctd_basic_branches_fwd_train: 1..%d branches", BR_MAX);
  for (int i = 0; i < nb * n; ++i)
    BUCTD_CHECK_ARG(fwd_ptrs_ok(blocks[i]), "buctd_basic_branches_fwd_train: null pointer in block %d", i);
  return row_fwd_train(true, nb, n, blocks, stream);
}
extern "C" int buctd_basic_branches_bwd(int nb, int n, const buctd_basic_block* blocks, const buctd_basic_block_grads* grads,
                                        void* stream, void* side_stream) {
  BUCTD_CHECK_ARG(nb > 0 && nb <= BR_MAX && n > 0 && blocks && grads, "buctd_basic_branches_bwd: 1..%d branches", BR_MAX);
  for (int i = 0; i < nb * n; ++i)
    BUCTD_CHECK_ARG(bwd_ptrs_ok(blocks[i], grads[i]), "buctd_basic_branches_bwd: null pointer in block %d", i);
  return row_bwd(true, "buctd_basic_branches_bwd", nb, n, blocks, grads, stream, side_stream);
}

/* `to` waits for everything enqueued on `from` so far: the fork in front of a weight gradient that the host mirror launches
 * on the side stream itself. */
extern "C" int buctd_stream_fork(void* from, void* to) {
  return stream_fork((hipStream_t)from, (hipStream_t)to, "buctd_stream_fork");
}
