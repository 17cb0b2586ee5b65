"""Host side of the fused policy kernel (csrc/fa_policy.hip): pack an MPNN's parameters (mpnn.py /
a reference state_dict) into the kernel's weight buffer.

Three pairs of consecutive linear maps of the reference network are multiplied out here, in float64,
and rounded to float32 once (exact in real arithmetic; fp32 rounding differs from evaluating the
factors one after the other by ~1e-6 relative -- the size of a GEMM's own summation-order noise):

    A_o = norm_o * oppAttn.W_key  @ oppAttn.W_query^T        scores_ij = (h1_i A_o) . ho_j
    B_o =          oppAttn.W_val  @ oppAttn.W_out            e_opp_i   = (sum_j a_ij ho_j) B_o
    A_m = norm   * messages.W_query @ messages.W_key^T       comp_ij   = (h_i A_m) . h_j
    W7  = [ update.weight[:, :128]^T ; messages.W_val @ messages.W_out @ update.weight[:, 128:]^T ]
                                                             h'        = relu([h | sum_j a_ij h_j] W7 + b)

`kernel_params` is the one statement of that algebra (any dtype, inside or outside autograd) and `SECTIONS` the one
statement of the buffers' layout: every offset below is a running sum over it (csrc/fa_policy.h and fa_train.h hold the
same numbers as FA_POFF_* / FA_POFF3_* / FA_TOFF_* and assert their own consistency; tests/test_abi_cpu.py compares the
two).  Dense operands are stored in the lane order of the 32x32x2 fp32 MFMA's B operand (`pack_gemm`).
`folded_forward` evaluates the packed buffer with plain torch ops (CPU or GPU): it is what the CPU tests compare with
MPNN.logits_value, and documents the kernel's arithmetic.
"""
import math

import torch

HIDDEN = 128
MAX_TEAM = 8
# The kernel-facing matrices in buffer order: (name, plain row-major shape, dense).  A dense one is an MFMA B operand: packed
# in the forward buffer (float32 lane order, then once more as bf16x3) and, transposed, in the backward's buffer.
SECTIONS = (("WE", (6, 64), False), ("BE", (64,), False), ("WOE", (6, 64), False), ("BOE", (64,), False),
            ("AO", (64, 64), True), ("BO", (64, 64), True), ("AM", (128, 128), True), ("W7", (256, 128), True),
            ("BU", (128,), False), ("W8", (128, 256), True), ("B8", (256,), False), ("W9", (256, 32), True), ("B9", (32,), False))
PLAIN_SHAPES = {k: shp for k, shp, _ in SECTIONS}
_GEMMS = tuple(k for k, _, dense in SECTIONS if dense)


def _offsets(sizes, at=0, align=1):
    """[(name, floats)] laid out back to back from `at` (each start rounded up to `align`) -> ({name: offset}, end)."""
    off = {}
    for k, n in sizes:
        at = -(-at // align) * align
        off[k] = at
        at += n
    return off, at


# the float32 sections = the layout of the plain / gradient buffers (FA_POFF_*, FA_POLICY_PLAIN_FLOATS) ...
POFF, PLAIN_FLOATS = _offsets((k, math.prod(shp)) for k, shp, _ in SECTIONS)
# ... followed by the dense matrices split into three bf16 terms, 1.5 floats per weight (FA_POFF3_*, FA_POLICY_WEIGHT_FLOATS)
POFF3, WEIGHT_FLOATS = _offsets(((k, math.prod(PLAIN_SHAPES[k]) * 3 // 2) for k in _GEMMS), PLAIN_FLOATS)
# the transposed pack of the PPO update's kernel (csrc/fa_train.h FA_TOFF_*, FA_TRANS_FLOATS) and its gradient slab
TOFF, TRANS_FLOATS = _offsets((k + "T", math.prod(PLAIN_SHAPES[k])) for k in _GEMMS)
SLAB_FLOATS = PLAIN_FLOATS + 16


def _rne_hi(x):
    """float32 tensor -> float32 tensor rounded to nearest-even at 8 significant bits (a bf16 in a float's clothes)."""
    u = x.contiguous().view(torch.int32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & -65536).view(torch.float32)


def pack_gemm3(w):
    """(K, C) matrix -> the bf16x3 B-operand pack as a flat float32 tensor of 1.5 K C floats: every weight (rounded to float32
    first) is EXACTLY hi + mid + lo, three bf16 numbers; 16-byte index ((cb * K/16 + s) * 3 + term) * 64 + lane holds the eight
    bf16 W[k = (lane >> 5) * K/2 + 8 s + j][col = 32 cb + (lane & 31)], j = 0..7 (csrc/fa_policy.h; fa_pack_weights writes the same)."""
    K, C = w.shape
    assert K % 16 == 0 and C % 32 == 0
    x = w.float().contiguous()
    hi = _rne_hi(x)
    r1 = x - hi
    mid = _rne_hi(r1)
    lo = r1 - mid
    terms = torch.stack([(t.contiguous().view(torch.int32) >> 16).to(torch.int16) for t in (hi, mid, lo)])   # (3, K, C) bf16 bits
    t = terms.reshape(3, 2, K // 16, 8, C // 32, 32).permute(4, 2, 0, 1, 5, 3).contiguous()                  # cb, s, term, hh, li, j
    return t.reshape(-1).view(torch.float32)


def pack_gemm(w):
    """(K, C) matrix -> flat float32 in B-operand order: float4 index (cb * K/8 + t4) * 64 + lane holds
    W[k = (lane >> 5) * K/2 + 4*t4 + q][col = 32*cb + (lane & 31)], q = 0..3."""
    K, C = w.shape
    assert K % 8 == 0 and C % 32 == 0
    return w.reshape(2, K // 8, 4, C // 32, 32).permute(3, 1, 0, 4, 2).contiguous().reshape(-1)


def unpack_gemm(flat, K, C):
    """Inverse of pack_gemm."""
    return flat.reshape(C // 32, K // 8, 2, 32, 4).permute(2, 1, 4, 0, 3).contiguous().reshape(K, C)


def unpack_gemm3(flat3, K, C):
    """Inverse of pack_gemm3: the (K, C) float32 matrix hi + mid + lo (exact: the split loses nothing)."""
    bits = flat3.contiguous().view(torch.int16).reshape(C // 32, K // 16, 3, 2, 32, 8).permute(2, 3, 1, 5, 0, 4).reshape(3, K, C)
    t = (bits.to(torch.int32) << 16).view(torch.float32)
    return (t[0] + t[1]) + t[2]


def supported(pol):
    return pol.h_dim == HIDDEN and pol.embed_dim == HIDDEN and pol.input_size == 6 and \
        pol.num_agents <= MAX_TEAM and pol.num_opp_agents <= MAX_TEAM and pol.dist.linear.out_features == 8


def kernel_params(pol, dtype=None, heads=True):
    """The matrices the fused kernels work with (the folded products of this file's header, the stacked heads, zero-padded
    W9 / b9), in the parameters' dtype or in `dtype`.  With gradients enabled they are INSIDE the autograd graph of the
    module's parameters: torch.autograd.backward on them with the kernel's gradients applies the chain rule to the
    parameters.  The scaled products are norm * (A @ B): what the device fold computes (FlatPolicy: alpha * acc).
    heads=False: the trunk's alone (MPNN.trunk_folded: any hidden size and number of actions)."""
    c = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    a, m, hd = pol.oppAttn, pol.messages, pol.h_dim
    uw = c(pol.update[0].weight)
    P = dict(
        WE=c(pol.encoder[0].weight).t(), BE=c(pol.encoder[0].bias),
        WOE=c(pol.oppEncoder[0].weight).t(), BOE=c(pol.oppEncoder[0].bias),
        AO=a.norm_factor * (c(a.W_key[0]) @ c(a.W_query[0]).t()), BO=c(a.W_val[0]) @ c(a.W_out[0]),
        AM=m.norm_factor * (c(m.W_query[0]) @ c(m.W_key[0]).t()),
        W7=torch.cat((uw[:, :hd].t(), (c(m.W_val[0]) @ c(m.W_out[0])) @ uw[:, hd:].t()), 0), BU=c(pol.update[0].bias))
    if heads:
        z = lambda *s: torch.zeros(*s, device=uw.device, dtype=uw.dtype)
        P.update(
            W8=torch.cat((c(pol.policy_head[0].weight).t(), c(pol.value_head[0].weight).t()), 1),
            B8=torch.cat((c(pol.policy_head[0].bias), c(pol.value_head[0].bias))),
            W9=torch.cat((torch.cat((c(pol.dist.linear.weight).t(), z(hd, 24)), 1),
                          torch.cat((z(hd, 8), c(pol.value_head[2].weight).t(), z(hd, 23)), 1)), 0),
            B9=torch.cat((c(pol.dist.linear.bias), c(pol.value_head[2].bias), z(23))))
    return P


@torch.no_grad()
def pack_from_params(P, out_fwd, out_t=None):
    """kernel_params() -> the forward pack (FA_POFF_*; its bf16x3 half when out_fwd has room for it) and, when asked for,
    the transposed pack (FA_TOFF_*), in place; rounded to float32 here, once."""
    for k in PLAIN_SHAPES:
        v = P[k].detach()
        flat = pack_gemm(v) if k in _GEMMS else v.reshape(-1)
        out_fwd[POFF[k]:POFF[k] + flat.numel()].copy_(flat)
        if k in _GEMMS and out_fwd.numel() >= WEIGHT_FLOATS:
            x3 = pack_gemm3(v)
            out_fwd[POFF3[k]:POFF3[k] + x3.numel()].copy_(x3)
        if k in _GEMMS and out_t is not None:
            flat = pack_gemm(v.t())
            out_t[TOFF[k + "T"]:TOFF[k + "T"] + flat.numel()].copy_(flat)


@torch.no_grad()
def pack_policy(pol, out=None):
    """MPNN module (mpnn.py) -> packed float32 buffer on the module's device, the fold evaluated in float64; `out` is
    rewritten in place when given (a captured hipGraph keeps pointing at it)."""
    if not supported(pol):
        raise ValueError("the fused policy kernel needs hidden_dim = 128, 6 inputs, 8 actions and teams of <= 8")
    P = kernel_params(pol, torch.float64)
    if out is None:
        out = torch.zeros(WEIGHT_FLOATS, dtype=torch.float32, device=P["W7"].device)
    assert out.numel() == WEIGHT_FLOATS and out.dtype == torch.float32 and out.is_contiguous()
    pack_from_params(P, out)
    return out


def split_plain(flat):
    """A plain-layout buffer (the float32 sections at the POFF offsets: a FA_SLAB of gradients) -> dict of views shaped
    like kernel_params()."""
    return {k: flat[POFF[k]:POFF[k] + math.prod(shp)].view(*shp) for k, shp in PLAIN_SHAPES.items()}


def _forward(P, own, opp):
    """The network on the kernel-facing matrices P: own (B, n, 6), opp (B, m, 6) -> (B, n, 32): 8 logits, the value, zeros."""
    n = own.shape[1]
    h1 = torch.relu(own @ P["WE"] + P["BE"])
    ho = torch.relu(opp @ P["WOE"] + P["BOE"])
    att = torch.softmax((h1 @ P["AO"]) @ ho.transpose(1, 2), dim=-1)              # (B, n, m)
    h = torch.cat((h1, (att @ ho) @ P["BO"]), dim=2)
    diag = torch.zeros(n, n, device=own.device).fill_diagonal_(-float("inf"))
    for _ in range(3):
        mix = torch.softmax((h @ P["AM"]) @ h.transpose(1, 2) + diag, dim=-1) @ h if n > 1 else torch.zeros_like(h)
        h = torch.relu(torch.cat((h, mix), dim=2) @ P["W7"] + P["BU"])
    return torch.relu(h @ P["W8"] + P["B8"]) @ P["W9"] + P["B9"]


@torch.no_grad()
def folded_forward(flat, own, opp):
    """The kernel's arithmetic on the packed buffer: own (B, n, 6), opp (B, m, 6) -> logits (B, n, 8), value (B, n, 1)."""
    P = {}
    for k, shp in PLAIN_SHAPES.items():
        sec = flat[POFF[k]:POFF[k] + math.prod(shp)]
        P[k] = unpack_gemm(sec, *shp) if k in _GEMMS else sec.view(*shp)
    out = _forward(P, own, opp)
    return out[..., :8], out[..., 8:9]


def folded_ppo_reference(P, obs, own_sl, opp_sl, action, value_pred, ret, old_logp, adv, clip, c_value, c_entropy,
                         clipped_value_loss=True):
    """Plain-torch statement of csrc/fa_train.hip (forward on the kernel-facing matrices P + the losses of
    ppo.py:146-187 WITHOUT the division by the mask mean): returns (loss, value_loss, action_loss, entropy, mask_mean)
    where loss = c_value * value_loss + action_loss - c_entropy * entropy; differentiable in P."""
    own = obs[:, own_sl]
    out = _forward(P, own, obs[:, opp_sl])
    logp_all = torch.log_softmax(out[..., :8], dim=-1)
    value = out[..., 8:9]
    mask = own[:, :, 0:1]
    logp = logp_all.gather(-1, action)
    ent = -(logp_all.exp() * logp_all).sum(-1, keepdim=True)
    ratio = mask * torch.exp(logp - old_logp)
    al = (mask * -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)).mean()
    if clipped_value_loss:
        vclip = value_pred + (value - value_pred).clamp(-clip, clip)
        vl = (0.5 * torch.max((value - ret).pow(2), (vclip - ret).pow(2)) * mask).mean()
    else:
        vl = 0.5 * (ret - value).pow(2).mean()
    en = (ent * mask).mean()
    return vl * c_value + al - en * c_entropy, vl, al, en, mask.mean()


# ---- the module's parameters as ONE flat buffer + the fold / unfold task lists (csrc/fa_fold.hip) -----------------
# (name, accessor, (rows, columns)) of what the forward uses (oppUpdate is created but never used, mpnn.py:44-45), in the
# order of the flat buffer; every parameter starts at a multiple of 4 floats
_PARAMS = (("ENC_W", lambda p: p.encoder[0].weight, (64, 6)), ("ENC_B", lambda p: p.encoder[0].bias, (1, 64)),
           ("OENC_W", lambda p: p.oppEncoder[0].weight, (64, 6)), ("OENC_B", lambda p: p.oppEncoder[0].bias, (1, 64)),
           ("OQ", lambda p: p.oppAttn.W_query, (64, 64)), ("OK", lambda p: p.oppAttn.W_key, (64, 64)),
           ("OV", lambda p: p.oppAttn.W_val, (64, 64)), ("OO", lambda p: p.oppAttn.W_out, (64, 64)),
           ("MQ", lambda p: p.messages.W_query, (128, 128)), ("MK", lambda p: p.messages.W_key, (128, 128)),
           ("MV", lambda p: p.messages.W_val, (128, 128)), ("MO", lambda p: p.messages.W_out, (128, 128)),
           ("UW", lambda p: p.update[0].weight, (128, 256)), ("UB", lambda p: p.update[0].bias, (1, 128)),
           ("V0W", lambda p: p.value_head[0].weight, (128, 128)), ("V0B", lambda p: p.value_head[0].bias, (1, 128)),
           ("V2W", lambda p: p.value_head[2].weight, (1, 128)), ("V2B", lambda p: p.value_head[2].bias, (1, 1)),
           ("P0W", lambda p: p.policy_head[0].weight, (128, 128)), ("P0B", lambda p: p.policy_head[0].bias, (1, 128)),
           ("DW", lambda p: p.dist.linear.weight, (8, 128)), ("DB", lambda p: p.dist.linear.bias, (1, 8)))
_PF_OFF, PF_FLOATS = _offsets(((k, r * c) for k, _, (r, c) in _PARAMS), align=4)
_PF = tuple((k, get, _PF_OFF[k]) for k, get, _ in _PARAMS)        # (name, accessor, offset in floats)

# The fold (this file's header) as data, on row-major matrices named as above: a parameter, a plain section (a vector is one
# row) or "M" = messages.W_val W_out, a scratch matrix; a block of one is (name, (row, column, rows, columns)).
_MATS = dict([(k, shp) for k, _, shp in _PARAMS] + [(k, shp if len(shp) == 2 else (1,) + shp) for k, shp, _ in SECTIONS],
             M=(128, 128))
# copies: (section, row, column) where the block starts <- parameter (block), transposed or not
_COPIES = (("WE", 0, 0, "ENC_W", True), ("BE", 0, 0, "ENC_B", False), ("WOE", 0, 0, "OENC_W", True), ("BOE", 0, 0, "OENC_B", False),
           ("W7", 0, 0, ("UW", (0, 0, 128, 128)), True), ("BU", 0, 0, "UB", False),
           ("W8", 0, 0, "P0W", True), ("W8", 0, 128, "V0W", True), ("B8", 0, 0, "P0B", False), ("B8", 0, 128, "V0B", False),
           ("W9", 0, 0, "DW", True), ("W9", 128, 8, "V2W", True), ("B9", 0, 0, "DB", False), ("B9", 0, 8, "V2B", False))
# products C = alpha * A op(B): (C, A, B, B transposed, whose norm_factor alpha is, row chunks = tasks)
_PRODUCTS = (("AO", "OK", "OQ", True, "oppAttn", 1), ("BO", "OV", "OO", False, None, 1), ("AM", "MQ", "MK", True, "messages", 4),
             ("M", "MV", "MO", False, None, 4), (("W7", (128, 0, 128, 128)), "M", ("UW", (0, 128, 128, 128)), True, None, 4))


def _ref(m):
    """A matrix or a block of one -> (name, float offset inside the matrix, rows, columns, leading dimension)."""
    name, blk = (m, None) if isinstance(m, str) else m
    r0, c0, r, c = blk or (0, 0) + _MATS[name]
    return name, r0 * _MATS[name][1] + c0, r, c, _MATS[name][1]


def _strides(ref, t):
    """(row, column) stride of op(matrix); one row has row stride 0."""
    _, _, r, c, ld = ref
    rs, cs = (ld if r > 1 else 0), 1
    if t:
        r, rs, cs = c, cs, rs
    return (0 if r == 1 else rs), cs


def _cp(Cp, c, Ap, a, t):
    """C = op(A): one copy task."""
    return dict(C=Cp, ldc=c[4], M=c[2], N=c[3], A=Ap, a=_strides(a, t))


def _mm(Cp, c, Ap, a, ta, Bp, b, tb, alpha, split):
    """C = alpha * op(A) op(B) as `split` row chunks (one task, FA_TASK_SLICES workgroups, each)."""
    sa, rows = _strides(a, ta), c[2] // split
    return [dict(C=Cp + 4 * s * rows * c[4], ldc=c[4], M=rows, N=c[3], K=a[2] if ta else a[3], A=Ap + 4 * s * rows * sa[0], a=sa,
                 B=Bp, b=_strides(b, tb), alpha=alpha) for s in range(split)]


class FlatPolicy(object):
    """An MPNN whose (used) parameters live in one flat device buffer `pflat` -- the module's tensors become views
    of it, their .grad views of `gflat` -- plus the task lists that turn `pflat` into the fused kernels' weight
    packs (`fold_pack`: 3 launches) and the kernel's plain-layout gradients into `gflat` (`unfold`: 2 launches):
    the folding algebra of this file's header and its chain rule, without a PyTorch op.  torch optimizers and
    clip_grad_norm_ work on the module's parameters as before."""

    @classmethod
    def of(cls, pol):
        """The FlatPolicy of `pol` (one per module: a second one would re-point the parameters away from the first)."""
        fp = pol.__dict__.get("_flat_policy")
        if fp is None or fp.pol is not pol or not fp.attached():
            fp = cls(pol)
            pol.__dict__["_flat_policy"] = fp
        return fp

    def attached(self):
        """Whether the module's parameters are still views of pflat (a .to() / .data assignment detaches them)."""
        base = self.pflat.data_ptr()
        return all(get(self.pol).data_ptr() == base + 4 * off for _, get, off in _PF)

    def __init__(self, pol):
        import ctypes as C
        from . import _lib
        if not supported(pol):
            raise ValueError("FlatPolicy needs hidden_dim = 128, 6 inputs, 8 actions and teams of <= 8")
        self.pol, self._lib, self._C = pol, _lib, C
        dev = pol.update[0].weight.device
        z = lambda n: torch.zeros(n, device=dev, dtype=torch.float32)
        self.pflat, self.gflat = z(PF_FLOATS), z(PF_FLOATS + 8)     # + 8: room for loss sums in one all-reduce
        with torch.no_grad():
            for name, get, off in _PF:
                p = get(pol)
                n = p.numel()
                self.pflat[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.pflat[off:off + n].view(p.shape)
        self.plain, self.mscr, self.dmscr = z(PLAIN_FLOATS), z(128 * 128), z(128 * 128)
        self.w, self.wt = z(WEIGHT_FLOATS), z(TRANS_FLOATS)
        self._fold = [self._tasks(s) for s in self._stages()]
        self._unfold = {}       # gradient buffer address -> its two task lists (captured graphs keep the pointers)
        self.attach_grads()

    def attach_grads(self):
        """(Re)point every parameter's .grad at its slice of gflat."""
        for name, get, off in _PF:
            p = get(self.pol)
            p.grad = self.gflat[off:off + p.numel()].view(p.shape)

    # -- task lists ---------------------------------------------------------------------------------------------
    def _tasks(self, items):
        C, L = self._C, self._lib
        arr = (L.Task * len(items))()
        for t, d in zip(arr, items):
            t.C, t.A, t.B = d["C"], d["A"], d.get("B", 0)
            t.ldc, t.M, t.N, t.K = d["ldc"], d["M"], d["N"], d.get("K", 1)
            t.a_rs, t.a_cs, t.b_rs, t.b_cs = d["a"][0], d["a"][1], d.get("b", (0, 0))[0], d.get("b", (0, 0))[1]
            t.alpha, t.type = d.get("alpha", 1.0), 0 if "B" in d else 1
        buf = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.pflat.device)
        return buf, len(items)

    def _run(self, tl):
        L, C = self._lib, self._C
        L.check(L.load().fa_run_tasks(tl[0].data_ptr(), tl[1], C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fa_run_tasks")

    def _stages(self, gp=None):
        """The two launches' task lists of the fold (pflat -> plain), or, given the address gp of plain-layout gradients, of
        its chain rule (gp -> gflat).  Stage 2 holds what reads the scratch that stage 1 writes: M (mscr), dM (dmscr)."""
        val = (self.pflat.data_ptr(), self.plain.data_ptr(), self.mscr.data_ptr())
        grd = (self.gflat.data_ptr(), gp, self.dmscr.data_ptr())

        def at(ref, grad=False):        # address of a matrix block, or of its gradient
            par, sec, scr = grd if grad else val
            name = ref[0]
            base = scr if name == "M" else sec + 4 * POFF[name] if name in POFF else par + 4 * _PF_OFF[name]
            return base + 4 * ref[1]

        back, st = gp is not None, ([], [])
        for sec, r0, c0, par, t in _COPIES:
            src = _ref(par)
            dst = _ref((sec, (r0, c0) + ((src[3], src[2]) if t else (src[2], src[3]))))
            # a copy's reverse is the (transposed) copy of the gradient
            st[0].append(_cp(at(src, True), src, at(dst, True), dst, t) if back else _cp(at(dst), dst, at(src), src, t))
        for C, A, B, tb, norm, split in _PRODUCTS:
            C, A, B = _ref(C), _ref(A), _ref(B)
            alpha = getattr(self.pol, norm).norm_factor if norm else 1.0
            if not back:
                st["M" in (A[0], B[0])].extend(_mm(at(C), C, at(A), A, False, at(B), B, tb, alpha, split))
                continue
            dC, out = at(C, True), st[C[0] == "M"]
            out.extend(_mm(at(A, True), A, dC, C, False, at(B), B, not tb, alpha, split))     # dA = alpha dC op(B)^T
            if tb:                                                                            # dB = alpha dC^T A ...
                out.extend(_mm(at(B, True), B, dC, C, True, at(A), A, False, alpha, split))
            else:                                                                             # ... or alpha A^T dC
                out.extend(_mm(at(B, True), B, at(A), A, True, dC, C, False, alpha, split))
        return st

    def fold_pack(self):
        """parameters -> plain kernel-facing matrices -> forward + transposed packs (self.w, self.wt)."""
        L, C = self._lib, self._C
        self._run(self._fold[0])
        self._run(self._fold[1])
        L.check(L.load().fa_pack_weights(self.plain.data_ptr(), self.w.data_ptr(), self.wt.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fa_pack_weights")
        return self.w, self.wt

    def _build_unfold(self, gp):
        """gp: data pointer of the plain-layout gradient buffer (the fa_ppo_grad slab sum)."""
        return [self._tasks(s) for s in self._stages(gp)]

    def unfold(self, grads_plain):
        """plain-layout gradients of the kernel-facing matrices (a FA_SLAB buffer) -> gflat (== every parameter's
        .grad): the chain rule of the fold.  Uses M = W_val W_out of the LAST fold_pack()."""
        tl = self._unfold.get(grads_plain.data_ptr())
        if tl is None:      # never dropped: every GraphedPPOStep's graph replays fa_task_kernel on ITS list
            tl = self._unfold[grads_plain.data_ptr()] = self._build_unfold(grads_plain.data_ptr()) + [grads_plain]
        self._run(tl[0])
        self._run(tl[1])

    # -- optimizer --------------------------------------------------------------------------------------------------
    def bind_adam(self, opt):
        """Make a torch.optim.Adam over this module keep its state in flat buffers (exp_avg / exp_avg_sq of every
        parameter = views of mflat / vflat, the step counters = views of `steps`), so adam_step() below and the
        optimizer's own step() advance the same state."""
        if getattr(self, "_opt", None) is opt:
            return
        g = opt.param_groups[0]
        assert len(opt.param_groups) == 1 and not g.get("amsgrad") and not g.get("weight_decay") and not g.get("maximize"), \
            "fa_adam_step is plain Adam: one group, no amsgrad / weight decay / maximize"
        dev = self.pflat.device
        self.mflat, self.vflat = torch.zeros_like(self.pflat), torch.zeros_like(self.pflat)
        self.steps = torch.zeros(len(_PF), device=dev, dtype=torch.float32)
        seg = []
        for k, (name, get, off) in enumerate(_PF):
            p = get(self.pol)
            n = p.numel()
            seg.append(off)
            st = opt.state[p]
            views = {"step": self.steps[k], "exp_avg": self.mflat[off:off + n].view(p.shape),
                     "exp_avg_sq": self.vflat[off:off + n].view(p.shape)}
            for key, view in views.items():
                if key in st and torch.is_tensor(st[key]):
                    view.copy_(st[key].to(dev))
                st[key] = view
        assert seg == sorted(seg) and seg[0] == 0
        self._seg = torch.tensor(seg + [PF_FLOATS], dtype=torch.int32, device=dev)
        self._coef = torch.zeros(int(self._lib.load().fa_adam_scratch_floats()), device=dev)   # [0]: the clip coefficient
        self._hyper = torch.zeros(8, device=dev)      # (lr, beta1, beta2, eps, max_grad_norm): refresh_hyper()
        self._hyper_host = None
        self._opt = opt

    def refresh_hyper(self, opt, max_grad_norm):
        """Bring the device copy of (lr, beta1, beta2, eps, max_grad_norm) up to date: fa_adam_step_dev reads them at run
        time, so a captured optimizer step follows a change of opt.param_groups[0] (copy only when something moved)."""
        self.bind_adam(opt)
        g = opt.param_groups[0]
        hp = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(max_grad_norm))
        if hp != self._hyper_host:
            self._hyper[:5].copy_(torch.tensor(hp, dtype=torch.float32))
            self._hyper_host = hp

    def adam_step(self, opt, max_grad_norm):
        """clip_grad_norm_(max_grad_norm) + Adam over the flat buffers: fa_adam_step_dev (two launches)."""
        if not torch.cuda.is_current_stream_capturing():
            self.refresh_hyper(opt, max_grad_norm)
        L, C = self._lib, self._C
        vp = lambda t: C.c_void_p(t.data_ptr())
        L.check(L.load().fa_adam_step_dev(vp(self.pflat), vp(self.gflat), vp(self.mflat), vp(self.vflat), vp(self.steps), vp(self._seg),
                                          len(_PF), PF_FLOATS, vp(self._hyper), vp(self._coef),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fa_adam_step_dev")
