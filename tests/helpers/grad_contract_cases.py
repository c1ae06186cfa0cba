"""Case table of the gradient contract of the autograd nodes (buctd_amd/ops.py, ops_seq.py): one entry per node that hands a
parameter gradient to ops.grad_target, built through the project's own module where one exists so that the module's dispatch
is under test too, next to a plain torch module of the same state_dict that serves as the fp32 / fp64 CPU reference.

A case: name, sites (the functions whose grad_target calls a backward of the case passes through, as `Class.method` or
`function`), build() -> Built, kind ("blocks": the bar of test_gpu_blocks.py, "attn": the 2e-5 of test_gpu_attention.py),
math (the conv math mode to run in), veto (ops.native_block_veto set: the step-by-step BasicBlockFn).
Importing this module needs no GPU and not the package: build() imports what it needs.

tests/test_grad_contract_cover.py holds the table against the source (every function that calls grad_target is named by a
case); tests/test_gpu_grad_contract.py runs it."""
import ast
import math
import os

import torch
import torch.nn as tnn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SOURCES = ("buctd_amd/ops.py", "buctd_amd/ops_seq.py")


# ---- the source: who calls grad_target ----------------------------------------------------------------------------------------
def grad_target_calls(sources=SOURCES, root=ROOT):
    """{(file name, line): qualified name of the function that calls grad_target on that line}"""
    calls = {}
    for rel in sources:
        with open(os.path.join(root, rel)) as f:
            tree = ast.parse(f.read())

        def walk(node, scope):
            for child in ast.iter_child_nodes(node):
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    walk(child, scope + [child.name])
                    continue
                if isinstance(child, ast.Call):
                    fn = child.func
                    name = fn.id if isinstance(fn, ast.Name) else fn.attr if isinstance(fn, ast.Attribute) else None
                    if name == "grad_target" and scope:
                        calls[(os.path.basename(rel), child.lineno)] = ".".join(scope)
                walk(child, scope)
        walk(tree, [])
    return calls


def functions_in_sources(sources=SOURCES, root=ROOT):
    """qualified names of every function of the sources"""
    names = set()
    for rel in sources:
        with open(os.path.join(root, rel)) as f:
            tree = ast.parse(f.read())

        def walk(node, scope):
            for child in ast.iter_child_nodes(node):
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    names.add(".".join(scope + [child.name]))
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    walk(child, scope + [child.name])
        walk(tree, [])
    return names


# ---- what a case builds -------------------------------------------------------------------------------------------------------
class Built:
    """ref: torch module (CPU, fp32); mod: the project's module with the same state_dict keys (CPU, not yet loaded);
    inputs: CPU fp32 tensors in the reference's layout; layout "nchw" (the device sees NHWC) or "tokens" (same on both);
    ref_fwd / mod_fwd(module, [inputs]) -> list of outputs; node: name of the grad_fn the first output must carry."""

    def __init__(self, ref, mod, inputs, layout="nchw", ref_fwd=None, mod_fwd=None, node=None):
        one = lambda m, xs: [m(xs[0])]      # noqa: E731
        self.ref, self.mod, self.inputs, self.layout = ref, mod, inputs, layout
        self.ref_fwd, self.mod_fwd, self.node = ref_fwd or one, mod_fwd or one, node


def _as_list(y):
    return list(y) if isinstance(y, (list, tuple)) else [y]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _shake(module, seed):
    """BatchNorm / LayerNorm affine parameters away from (1, 0), so that a dropped gamma or beta shows"""
    g = _gen(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (tnn.modules.batchnorm._BatchNorm, tnn.LayerNorm)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return module


# ---- conv + BatchNorm (+ ReLU) ------------------------------------------------------------------------------------------------
def conv_bn(N, H, W, ci, co, k, stride, relu, bias=False):
    def build():
        from buctd_amd import nn as bnn
        torch.manual_seed(ci * 100 + co + k)
        mods = [tnn.Conv2d(ci, co, k, stride, (k - 1) // 2, bias=bias), tnn.BatchNorm2d(co)] + ([tnn.ReLU()] if relu else [])
        ref = _shake(tnn.Sequential(*mods), 1)
        mod = bnn.ConvBN(bnn.Conv2d(ci, co, k, stride, (k - 1) // 2, bias=bias), bnn.BatchNorm2d(co),
                         bnn.ReLU(True) if relu else None)
        return Built(ref, mod, [torch.randn(N, ci, H, W, generator=_gen(2))], node="ConvBnActBackward")
    return build


def deconv_bn():
    """the transposed path of ConvBnAct: nn.conv_bn_act on a ConvTranspose2d (4x4, stride 2, as the deconvolution heads)"""
    def build():
        from buctd_amd import nn as bnn

        class Deconv(bnn.Sequential):
            def forward(self, x):
                return bnn.conv_bn_act(x, self[0], self[1], relu=True)
        torch.manual_seed(44)
        ref = _shake(tnn.Sequential(tnn.ConvTranspose2d(32, 16, 4, 2, 1, 0, bias=False), tnn.BatchNorm2d(16), tnn.ReLU()), 3)
        mod = Deconv(bnn.ConvTranspose2d(32, 16, 4, 2, 1, 0, bias=False), bnn.BatchNorm2d(16))
        return Built(ref, mod, [torch.randn(2, 32, 6, 5, generator=_gen(4))], node="ConvBnActBackward")
    return build


# ---- residual blocks ----------------------------------------------------------------------------------------------------------
def basic_block(shape):
    def build():
        from oracle import models as om
        from buctd_amd.models import hrnet_common as hc
        N, H, W, Cn = shape
        torch.manual_seed(N * H + Cn)
        return Built(_shake(om.BasicBlock(Cn, Cn), 5), hc.BasicBlock(Cn, Cn), [torch.randn(N, Cn, H, W, generator=_gen(6))],
                     node="BasicBlockFnBackward")
    return build


def basic_chain(N, H, W, Cn, n):
    def build():
        from oracle import models as om
        from buctd_amd.models import hrnet_common as hc
        torch.manual_seed(Cn + n)
        ref, _ = om.make_layer(om.BasicBlock, Cn, Cn, n)
        mod, _ = hc.make_residual_layer(hc.BasicBlock, Cn, Cn, n)
        return Built(_shake(ref, 7), mod, [torch.randn(N, Cn, H, W, generator=_gen(8))], node="BasicChainFnBackward")
    return build


def bottleneck(downsample):
    def build():
        from oracle import models as om
        from buctd_amd.models import hrnet_common as hc
        torch.manual_seed(64 + downsample)
        cin = 64 if downsample else 256
        ref, _ = om.make_layer(om.Bottleneck, cin, 64, 1)
        mod, _ = hc.make_residual_layer(hc.Bottleneck, cin, 64, 1)
        assert (mod[0].downsample is not None) == downsample
        return Built(_shake(ref, 9), mod, [torch.randn(2, cin, 12, 8, generator=_gen(10))], node="BottleneckFnBackward")
    return build


def fork():
    """the first transition of HRNet as one node: two conv + BN + ReLU heads on one input"""
    def build():
        from oracle import models as om
        from buctd_amd.models import hrnet_common as hc
        torch.manual_seed(13)
        ref = tnn.Module()
        ref.transition1 = _shake(om.make_transition([64], [16, 32]), 11)
        trunk = hc.HRNetTrunk()
        trunk.transition1 = hc.make_transition_layer([64], [16, 32])
        trunk.stage2_cfg = {"NUM_BRANCHES": 2}
        return Built(ref, trunk, [torch.randn(2, 64, 12, 8, generator=_gen(12))],
                     ref_fwd=lambda m, xs: [m.transition1[0](xs[0]), m.transition1[1](xs[0])],
                     mod_fwd=lambda m, xs: _as_list(m.enter_stage(2, xs[0], first=True)), node="ForkConvBnFnBackward")

    return build


def hr_module(nb, branches_only=False):
    """HighResolutionModule with two blocks per branch at 32 / 64 (/ 128) channels: the widths from which all branches share
    one group-launch family (ops.group_branches_ok), on 12x8 and smaller maps.  branches_only: the branches alone, whose
    outputs are the outputs of ops.BasicBranchesFn itself (so that one of them can stay out of the loss)."""
    def build():
        from oracle import models as om
        from buctd_amd.models import hrnet_common as hc
        torch.manual_seed(nb)
        ch = [32 * 2 ** i for i in range(nb)]
        ref = _shake(om.HighResolutionModule(nb, om.BasicBlock, [2] * nb, list(ch), list(ch), "SUM", True), 13)
        mod = hc.HighResolutionModule(nb, hc.BasicBlock, [2] * nb, list(ch), list(ch), "SUM", True)
        xs = [torch.randn(2, ch[i], 12 >> i, 8 >> i, generator=_gen(14 + i)) for i in range(nb)]
        if branches_only:
            return Built(ref, mod, xs, ref_fwd=lambda m, x: [b(t) for b, t in zip(m.branches, x)],
                         mod_fwd=lambda m, x: _as_list(m._branches_grouped(x)), node="BasicBranchesFnBackward")
        return Built(ref, mod, xs, ref_fwd=lambda m, x: _as_list(m(list(x))), mod_fwd=lambda m, x: _as_list(m(list(x))),
                     node="FuseSumBackward")
    return build


# ---- plain convolution / linear ------------------------------------------------------------------------------------------------
def conv_bias():
    def build():
        from buctd_amd import nn as bnn
        torch.manual_seed(17)
        return Built(tnn.Conv2d(16, 8, 3, 1, 1), bnn.Conv2d(16, 8, 3, 1, 1), [torch.randn(2, 16, 9, 7, generator=_gen(18))],
                     node="ConvBackward")
    return build


# ---- attention and sequence nodes: function-style, wrapped in modules of the same parameter names --------------------------------
class _ChannelAttnRef(tnn.Module):
    """SimplifiedScaledDotProductAttention + fc_o on channel-major queries: the fp64 formula of test_gpu_attention.py"""

    def __init__(self, T, h, seed):
        super().__init__()
        g = _gen(seed)
        self.h = h
        self.fc_w = tnn.Parameter(torch.randn(T, T, generator=g) / math.sqrt(T))
        self.fc_b = tnn.Parameter(torch.randn(T, generator=g))

    def forward(self, qn, yn):
        B, T, Cn = yn.shape
        h, dk = self.h, T // self.h
        qc, yc = qn.permute(0, 2, 1), yn.permute(0, 2, 1)
        qh = qc.reshape(B, Cn, h, dk).permute(0, 2, 1, 3)
        kh = yc.reshape(B, Cn, h, dk).permute(0, 2, 3, 1)
        vh = yc.reshape(B, Cn, h, dk).permute(0, 2, 1, 3)
        att = torch.softmax(torch.matmul(qh, kh) / math.sqrt(dk), -1)
        out = torch.matmul(att, vh).permute(0, 2, 1, 3).contiguous().view(B, Cn, h * dk)
        return torch.nn.functional.linear(out, self.fc_w, self.fc_b).permute(0, 2, 1)


class _ChannelAttnMod(_ChannelAttnRef):
    def forward(self, qn, yn):
        from buctd_amd import ops
        assert ops.fc_o_x6_ok(yn.shape[1], yn.shape[0] * yn.shape[2]) == (yn.shape[1] == 576), "not the fc_o route of the case"
        return ops.ChannelAttention.apply(qn, yn, self.fc_w, self.fc_b, self.h, 0.0, False)


def channel_attention(B, T, Cn, h):
    def build():
        g = _gen(B * 77 + T)
        xs = [torch.randn(B, T, Cn, generator=g), torch.randn(B, T, Cn, generator=g)]
        two = lambda m, x: [m(x[0], x[1])]      # noqa: E731
        return Built(_ChannelAttnRef(T, h, T), _ChannelAttnMod(T, h, T), xs, "tokens", two, two, "ChannelAttentionBackward")
    return build


class _SmallQKRef(tnn.Module):
    """fc_q -> softmax(q k^T / sqrt(C)) -> . v (self_attention.py:74-86, h = 1)"""

    def __init__(self, d, Cn, seed):
        super().__init__()
        g = _gen(seed)
        self.wq = tnn.Parameter(torch.randn(Cn, d, generator=g))
        self.bq = tnn.Parameter(torch.randn(Cn, generator=g))

    def forward(self, yq, k, v):
        q = torch.nn.functional.linear(yq, self.wq, self.bq)
        return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(1, 2)) / math.sqrt(k.shape[2]), -1), v)


class _SmallQKMod(_SmallQKRef):
    def forward(self, yq, k, v):
        from buctd_amd import ops
        assert ops.attn_smallqk_ok(yq.shape[1], yq.shape[2], k.shape[2])
        return ops.SmallQKAttention.apply(yq, self.wq, self.bq, k, v, 0.0, False)


def smallqk(B, T, d, Cn):
    def build():
        g = _gen(B * 1000 + T + d)
        xs = [torch.randn(B, T, d, generator=g), torch.randn(B, T, Cn, generator=g), torch.randn(B, T, Cn, generator=g)]
        three = lambda m, x: [m(*x)]      # noqa: E731
        return Built(_SmallQKRef(d, Cn, 3), _SmallQKMod(d, Cn, 3), xs, "tokens", three, three, "SmallQKAttentionBackward")
    return build


class _AddLnRef(tnn.Module):
    def __init__(self, d):
        super().__init__()
        self.ln = tnn.LayerNorm(d)

    def forward(self, a, b):
        return self.ln(a + b)


class _AddLnMod(_AddLnRef):
    def forward(self, a, b):
        from buctd_amd import ops, ops_seq
        return ops_seq.AddLayerNorm.apply(a, b, self.ln, ops.grad_anchor(self.ln.parameters()))


def add_layernorm(B, T, d):
    def build():
        g = _gen(T + d)
        xs = [torch.randn(B, T, d, generator=g), torch.randn(B, T, d, generator=g)]
        two = lambda m, x: [m(x[0], x[1])]      # noqa: E731
        torch.manual_seed(d)
        return Built(_shake(_AddLnRef(d), 19), _AddLnMod(d), xs, "tokens", two, two, "AddLayerNormBackward")
    return build


class _InProjRef(tnn.Module):
    """nn.MultiheadAttention's input projection with q = k = qin, v = src (transpose_h.py:192-197)"""

    def __init__(self, d, seed):
        super().__init__()
        g = _gen(seed)
        self.w = tnn.Parameter(torch.randn(3 * d, d, generator=g) / math.sqrt(d))
        self.b = tnn.Parameter(torch.randn(3 * d, generator=g) * 0.1)

    def forward(self, qin, src):
        d = self.w.shape[1]
        lin = torch.nn.functional.linear
        return [lin(qin, self.w[: 2 * d], self.b[: 2 * d]), lin(src, self.w[2 * d:], self.b[2 * d:])]


class _InProjMod(_InProjRef):
    def forward(self, qin, src):
        from buctd_amd import ops_seq
        return list(ops_seq.InProjection.apply(qin, src, self.w, self.b))


def in_projection(B, T, d):
    def build():
        g = _gen(T * d)
        xs = [torch.randn(B, T, d, generator=g), torch.randn(B, T, d, generator=g)]
        two = lambda m, x: m(x[0], x[1])      # noqa: E731
        return Built(_InProjRef(d, 5), _InProjMod(d, 5), xs, "tokens", two, two, "InProjectionBackward")
    return build


class _AddPosRef(tnn.Module):
    """a learnable position embedding added in two encoder layers of one pass: its gradient is the sum of two pieces"""

    def __init__(self, T, d, seed):
        super().__init__()
        self.pos = tnn.Parameter(torch.randn(T, d, generator=_gen(seed)))

    def add(self, x):
        return x + self.pos

    def forward(self, x):
        return self.add(self.add(x) * 0.5)


class _AddPosMod(_AddPosRef):
    def add(self, x):
        from buctd_amd import ops_seq
        return ops_seq.add_pos(x, self.pos)

    def forward(self, x):
        from buctd_amd import ops_seq
        ops_seq.AddPos.begin(self.pos)
        return super().forward(x)


def add_pos(B, T, d):
    def build():
        return Built(_AddPosRef(T, d, 7), _AddPosMod(T, d, 7), [torch.randn(B, T, d, generator=_gen(T))], "tokens",
                     node="AddPosBackward")
    return build


# ---- the table ----------------------------------------------------------------------------------------------------------------
def case(name, sites, build, kind="blocks", math="bf16x6", veto=False):
    return dict(name=name, sites=tuple(sites), build=build, kind=kind, math=math, veto=veto)


CBA = "ConvBnAct.backward"
CASES = [
    case("convbn 3x3 s1 relu", [CBA], conv_bn(3, 12, 8, 16, 16, 3, 1, True)),
    case("convbn 3x3 s2", [CBA], conv_bn(3, 6, 5, 64, 128, 3, 2, False)),
    case("convbn 1x1", [CBA], conv_bn(3, 12, 8, 64, 16, 1, 1, False)),
    case("convbn 1x1 relu", [CBA], conv_bn(2, 5, 7, 32, 48, 1, 1, True)),
    case("convbn 3x3 conv bias", [CBA], conv_bn(2, 9, 7, 16, 32, 3, 1, True, bias=True)),
    case("convbn transposed", [CBA], deconv_bn()),
    case("basic block native 48", ["_block_grads"], basic_block((2, 12, 9, 48))),
    case("basic block native 96", ["_block_grads"], basic_block((3, 6, 5, 96))),
    case("basic block step by step", ["BasicBlockFn.backward"], basic_block((2, 12, 9, 48)), veto=True),
    case("basic block fp32", ["BasicBlockFn.backward"], basic_block((3, 6, 5, 96)), math="fp32"),
    case("basic chain of 4", ["_block_grads"], basic_chain(3, 12, 8, 32, 4)),
    case("bottleneck", [CBA], bottleneck(False)),
    case("bottleneck downsample", [CBA], bottleneck(True)),
    case("fork conv bn", [CBA], fork()),
    case("hr module 2 branches", ["_block_grads", CBA], hr_module(2)),
    case("hr module 3 branches", ["_block_grads", CBA], hr_module(3)),
    case("branches alone", ["_block_grads"], hr_module(2, branches_only=True)),
    case("conv bias", ["Conv.backward"], conv_bias()),
    case("channel attention", ["ChannelAttention.backward"], channel_attention(2, 96, 16, 1), kind="attn"),
    case("channel attention x6 fc_o", ["ChannelAttention.backward"], channel_attention(2, 576, 96, 1), kind="attn"),
    case("smallqk attention", ["SmallQKAttention.backward"], smallqk(2, 128, 3, 48), kind="attn"),
    case("add layernorm", ["AddLayerNorm.backward"], add_layernorm(2, 96, 16), kind="attn"),
    case("in projection", ["InProjection.backward"], in_projection(2, 96, 16), kind="attn"),
    case("add pos", ["AddPos.backward"], add_pos(2, 96, 16), kind="attn"),
]
BY_NAME = {c["name"]: c for c in CASES}
MULTI_OUTPUT = ("fork conv bn", "branches alone")        # the cases whose outputs are the outputs of ONE multi-output node
MIXED_NORM = ("convbn 3x3 s1 relu", "basic block native 48", "basic block step by step", "add layernorm")


# ---- frozen subsets ------------------------------------------------------------------------------------------------------------
def norm_names(module):
    out = []
    for mn, m in module.named_modules():
        if isinstance(m, (tnn.modules.batchnorm._BatchNorm, tnn.LayerNorm)):
            out += [(mn + "." if mn else "") + k for k, _ in m.named_parameters(recurse=False)]
    return out


def frozen_subsets(ref):
    """{tag: names to freeze}: every norm affine parameter | every convolution / linear weight | the first weight only |
    everything but the last parameter (in a chain: one of the last block).  Empty or repeated subsets are left out."""
    names = [k for k, _ in ref.named_parameters()]
    norms = set(norm_names(ref))
    weights = [k for k, p in ref.named_parameters() if p.dim() >= 2 and k not in norms]
    out, seen = {}, set()
    for tag, sub in (("norm affine", [k for k in names if k in norms]), ("weights", weights), ("first weight", weights[:1]),
                     ("all but one", names[:-1])):
        key = tuple(sub)
        if sub and key not in seen:
            seen.add(key)
            out[tag] = sub
    return out
