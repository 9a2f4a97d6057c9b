"""The ConvGRU fuser of the TRAINING step as one autograd node (`ops.gru_fuse` through ops.__getattr__).  _GruFuse does what every
route shares (dense views, weight packs, the gates' coordinate part; the seed view's gradient, the weight / bias gradients); the
walk over the views is one of two recurrences (_ring_route picks), each keeping its saved activations as its own attributes:
    forward(zz, base) -> (out, zz as the backward reads it)          backward(g, zz, need_z, need_w) -> (gz, g_seed, gwb, acc)
gwb: weight-gradient blocks [step | chunk][gate][z | state][27][16][16]; acc: the three gate gradients summed over the views.
The switches (GRU_RING, GRU_WGRAD_CHUNK, WGRAD_STREAM) are read as ops_train.NAME at call time."""
import collections
import functools

import torch

from . import _lib, ops, ops_train
from .ops import (_cached, _dense_views, _f32, _wsrc, cl, conv3d_c16_ring_bf16_io, conv3d_c16_wino, empty_cl, empty_cl16, he_constant,
                  launch, pack_conv3d_c16_ring_bf16, pack_conv3d_c16_wino, round_bf16)
from .ops_train import _SideWgrad, _Wgrad, bias_grad, conv_bwd_weight, ring_multi, ring_multi_ok

# The weight packs of the three gates: pk.<u | r | o>.<z | coords | state>.<fwd | t> -- the gate (update, reset, out), the 16
# input channels of its 35 that the pack convolves (the view, the zero-padded coordinates, the state), forward or transposed.
_Pack = collections.namedtuple('_Pack', 'fwd t')
_GatePacks = collections.namedtuple('_GatePacks', 'z coords state')
_Gates = collections.namedtuple('_Gates', 'u r o')


def _gate_packs(w, ac):
    def make():
        wd = _wsrc(w).detach()
        wc = wd.new_zeros(16, 16, 3, 3, 3)
        wc[:, :3] = wd[:, 16:19]
        pk = pack_conv3d_c16_ring_bf16 if ac else pack_conv3d_c16_wino
        return _GatePacks(*(_Pack(pk(t), pk(t, transpose=True)) for t in (wd[:, :16].contiguous(), wc, wd[:, 19:].contiguous())))
    return _cached(w, 'gru_fuse' + ('@ac' if ac else ''), make)


def _one(pack):                                                   # a ring-kernel pack as ring_multi's one-group stack
    return pack.reshape(1, 14, 16, 32)


def _gru_conv(ac, he, x, pack, addend=None, bias=None, out=None, out16=False, rnd=0):
    """One 16 -> 16 convolution of the per-gate path of _GruFuse: the bf16 ring kernel under the autocast policy (`ac`), the
    fp32 Winograd kernel otherwise; `addend` selects the addend form."""
    if ac:
        return conv3d_c16_ring_bf16_io(x, pack, bias, he, 0, rnd if addend is None else 0, addend=addend, out=out, out_bf16=out16)[0]
    prev = None if addend is None else (addend, None, _lib.LF_EPI_ADD)
    return conv3d_c16_wino(x, pack, bias, he, 0, prev=prev, out=out)[0]


def _gru_weight_grads(ctx, gwb, acc, c16, ws, he, ac):
    """The (weight, bias) gradients of the three gates from the per-step / per-chunk blocks gwb [*][gate][z | state][27][16][16]
    (summed in a fixed order) and the gate gradients' sums over the views acc[gate] (coordinate channels, bias)."""
    outs = []
    gsum = gwb.sum(dim=0)                                     # [gate][z | state][27][16][16]
    for k, w in enumerate(ws):
        gwt = torch.empty(27, 16, w.shape[1], device=gwb.device, dtype=torch.float32)
        gwt[:, :, :16] = gsum[k, 0]
        gwt[:, :, 19:] = gsum[k, 1]
        gc_, _ = conv_bwd_weight(c16, acc[k], 3, 16, he, want_bias=False, bf16=ac)
        gwt[:, :, 16:19] = gc_[:, :, :3]
        gw = gwt.reshape(3, 3, 3, 16, w.shape[1]).permute(3, 4, 0, 1, 2).contiguous()
        if ac:
            gw = round_bf16(gw)
        outs.append(gw if ctx.needs_input_grad[2 + 2 * k] else None)
        outs.append(bias_grad(acc[k], 3) if (ctx.has_bias[k] and ctx.needs_input_grad[3 + 2 * k]) else None)
    return outs


def _ring_route(ac, V, D, H, W):
    """The ring recurrence takes: autocast, at least one step, a volume ring_multi takes and a one-step chunk of which is in the
    bf16 weight-gradient kernel's domain (include/lf_hip.h: the generic kernel reads fp32, the ring recurrence stores bf16)."""
    return bool(ops_train.GRU_RING and ac and V >= 2 and ring_multi_ok(D, H, W) and D * H * W >= 8192)


class _Recurrence:
    def __init__(self, ac, he, pk):
        self.ac, self.he, self.pk = ac, he, pk


class _StepRecurrence(_Recurrence):
    """Round 5: per step six one-output convolutions (the addend form chains a gate's parts) and two stage kernels each way; the
    six weight gradients of a step beside the next steps' data gradients.  fp32, or bf16 storage of the once-per-step tensors
    under autocast (`ac`).  Saved: the step tensors `steps`, the states `hs` = h_1 .. h_{V-2}, `h0` when view 0 is not fp32."""

    def forward(self, zz, base):
        T16, pk = self.ac, self.pk                                # (T16: bf16 storage of the once-per-step tensors)
        conv = functools.partial(_gru_conv, self.ac, self.he)
        n = zz[0].numel()
        hs, saved = [_f32(zz[0:1])], []                           # (the state is fp32; view 0 seeds it)
        for i in range(1, zz.shape[0]):
            zi, h = zz[i:i + 1], hs[-1]
            upre, rpre = (conv(h, gate.state.fwd, addend=conv(zi, gate.z.fwd, addend=b, out16=T16), out16=T16)
                          for gate, b in ((pk.u, base[0]), (pk.r, base[1])))
            rh = empty_cl16(h.shape, h.device, T16)
            launch('lf_gru_train_stage_a', rpre, h, rh, n, int(T16))
            cand = conv(rh, pk.o.state.fwd, addend=conv(zi, pk.o.z.fwd, addend=base[2], out16=T16), out16=T16)
            hn = empty_cl(h.shape, h.device)
            launch('lf_gru_train_stage_b', h, upre, cand, hn, n, int(T16))
            saved.append((upre, rpre, rh, cand))
            hs.append(hn)
        self.steps = saved
        self.hs = hs[1:-1]                                        # h_1 .. h_{V-2}
        self.h0 = hs[0] if zz.dtype != torch.float32 else None    # (fp32 storage: h_0 is a view of z, which the node saves)
        return (hs[-1].clone() if zz.shape[0] == 1 else hs[-1]), zz

    def backward(self, g, zz, need_z, need_w):
        ac, T16, he, pk = self.ac, self.ac, self.he, self.pk
        V, dev, (D, H, W), n = zz.shape[0], zz.device, zz.shape[2:], zz[0].numel()
        shape1 = (1,) + tuple(zz.shape[1:])
        conv = functools.partial(_gru_conv, ac, he)
        gz = empty_cl16((V, 16, D, H, W), dev, zz.dtype == torch.bfloat16) if need_z else None
        acc = [empty_cl(shape1, dev).zero_() for _ in range(3)] if need_w else [None] * 3
        # weight-gradient blocks [step][gate][z | state][27][16][16], summed over the steps at the end (fixed order)
        gwb = torch.zeros(max(V - 1, 1), 3, 2, 27, 16, 16, device=dev, dtype=torch.float32) if need_w else None
        wg = _Wgrad(3, 1, D, H, W, 16, 16, dev, he, bf16=ac) if need_w else None      # (one scratch: the launches are in order)

        def weight_grads(i, zi, h, rh, gupre, grpre, gc):
            for k, (xh, gp) in enumerate(((h, gupre), (h, grpre), (rh, gc))):
                for q, x in enumerate((zi, xh)):
                    if ac and wg.entry != _Wgrad.BF16:            # small volumes: the fp32-MFMA kernel on the same bf16 values
                        wg(round_bf16(x.float()), round_bf16(gp.float()), gwb[i - 1, k, q])
                    else:
                        wg(x, gp, gwb[i - 1, k, q])
        gh1, gh12 = empty_cl(shape1, dev), empty_cl(shape1, dev)
        grh = empty_cl16(shape1, dev, T16)
        # the six weight gradients of a step run on the side stream (WGRAD_STREAM) beside the data-gradient chain; the gate
        # gradients they read are double-buffered, a buffer is rewritten only after the launches that read it have finished
        sw = _SideWgrad(dev, need_w)
        gbuf = [tuple(empty_cl16(shape1, dev, T16) for _ in range(3)) for _ in range(2 if sw.on else 1)]
        gdone = [None, None]
        if sw.on:
            sw.begin(gwb, wg.scratch, zz, *(b for bb in gbuf for b in bb))
        steps, hs = self.steps, self.hs
        for i in range(V - 1, 0, -1):
            gupre, gc, grpre = gbuf[i & 1 if sw.on else 0]
            sw.wait(gdone[i & 1])
            if steps[i - 1] is None:
                raise RuntimeError('the fused GRU recurrence frees its activations during backward: a second backward through '
                                   'the same graph is not supported')
            upre, rpre, rh, cand = steps[i - 1]
            h = (self.h0 if self.h0 is not None else zz[0:1]) if i == 1 else hs[i - 2]
            zi = zz[i:i + 1]
            launch('lf_gru_train_stage_b_bwd', g, h, upre, cand, gh1, gupre, gc, acc[0], acc[2], n, int(T16))
            conv(gc, pk.o.state.t, out=grh, rnd=1)
            launch('lf_gru_train_stage_a_bwd', grh, rpre, h, gh1, grpre, gh12, acc[1], n, int(T16))
            if need_w:                                            # the three gate gradients of this step are complete
                gdone[i & 1] = sw.run(functools.partial(weight_grads, i, zi, h, rh, gupre, grpre, gc), h, rh)
            if need_z:
                gzi = gz[i:i + 1]
                conv(gc, pk.o.z.t, out=gzi, rnd=1)
                conv(gupre, pk.u.z.t, addend=gzi, out=gzi)
                conv(grpre, pk.r.z.t, addend=gzi, out=gzi)
            gnext = empty_cl(shape1, dev)
            conv(gupre, pk.u.state.t, addend=gh12, out=gnext)
            conv(grpre, pk.r.state.t, addend=gnext, out=gnext)
            g = gnext
            steps[i - 1] = None                                   # the step's tensors are dead: free them as the walk goes
            if i >= 2:
                hs[i - 2] = None
        sw.join()
        return gz, g, gwb, acc


class _RingRecurrence(_Recurrence):
    """Round 6: the ring kernels with fused epilogues (csrc/conv_gru.hip), one output per launch on the chain.  The per-step
    tensors are STACKED blocks [V-1]: UP / RP / CA are first filled with the state-independent parts of the three gates (one
    launch over all views per gate), then overwritten in place by the pre-activations / the candidate of their step; the backward
    overwrites them once more with the gate GRADIENTS, which the weight gradients then read as multi-volume launches -- no per-step
    allocation, no element-wise stage launch in the forward.  Saved: `blocks` = UP, RP, CA, RH (r h), HS = fp32 h_0 .. h_{V-2}."""

    def forward(self, zz, base):
        he, pk = self.he, self.pk
        V, _, D, H, W = zz.shape
        self.z32 = zz.dtype != torch.bfloat16
        z_in = zz
        if self.z32:                                              # (the convolutions round x to bf16 while staging anyway: same numbers)
            zz = zz.to(torch.bfloat16)
        blk = lambda: empty_cl16((V - 1, 16, D, H, W), zz.device, True)      # noqa: E731
        UP, RP, CA, RH = blk(), blk(), blk(), blk()
        HS = empty_cl((V - 1, 16, D, H, W), zz.device)            # h_0 .. h_{V-2} (fp32 state)
        HS[0:1].copy_(z_in[0:1])                                  # (h_0 = view 0, un-rounded when the stack is fp32)
        for gate, dst, b in zip(pk, (UP, RP, CA), base):
            ring_multi(zz[1:], _one(gate.z.fwd), he, [(dst, b, False)], addend_per_sample=False)
        out = empty_cl(HS[0:1].shape, zz.device)
        for i in range(1, V):
            h, j = HS[i - 1:i], slice(i - 1, i)
            ring_multi(h, _one(pk.u.state.fwd), he, [(UP[j], UP[j], False)])
            ring_multi(h, _one(pk.r.state.fwd), he, [(RP[j], RP[j], False)], extra=_lib.LF_RING_EX_RH, o2=RH[j])
            hn = HS[i:i + 1] if i < V - 1 else out
            launch('lf_conv3d_c16_ring_blend', RH[j], _one(pk.o.state.fwd), CA[j], CA[j], h, UP[j], hn, None, 1, D, H, W, he,
                   tag='conv3d_c16_ring_multi', detail='1:2:1:11:2')
        self.blocks = [UP, RP, CA, RH, HS]
        return out, zz

    def backward(self, g, zz, need_z, need_w):
        """Per step ONE element-wise launch (lf_gru_train_stage_b_bwd, gate gradients written over the saved pre-activations) and
        three convolutions towards the state (gc -> g_rh with the reset gate's backward in its epilogue, gupre -> g_h = gh12 +,
        grpre -> g_h +=); the views' gradients follow the loop, three launches over the stored gate gradients of all steps.  The
        weight gradients run over the same blocks in chunks of GRU_WGRAD_CHUNK steps on the side stream beside the chain; the sums
        over the steps that the bias / coordinate-channel gradients need come from lf_sum_views_bf16."""
        if self.blocks is None:
            raise RuntimeError('the fused GRU recurrence overwrites its activations during backward: a second backward through '
                               'the same graph is not supported')
        (UP, RP, CA, RH, HS), self.blocks = self.blocks, None
        he, pk = self.he, self.pk
        V, dev, (D, H, W), n = zz.shape[0], zz.device, zz.shape[2:], zz[0].numel()
        shape1 = (1,) + tuple(zz.shape[1:])
        gz = empty_cl16((V, 16, D, H, W), dev, True)
        gh1, gh12 = empty_cl(shape1, dev), empty_cl(shape1, dev)
        gbuf = [empty_cl(shape1, dev), empty_cl(shape1, dev)]
        ends = list(range(V, 1, -ops_train.GRU_WGRAD_CHUNK if ops_train.GRU_WGRAD_CHUNK > 0 else -V)) + [1]
        chunks = list(zip(ends[1:], ends[:-1]))                   # (first step, one past the last step) in launch order
        gwb = torch.zeros(len(chunks), 3, 2, 27, 16, 16, device=dev, dtype=torch.float32) if need_w else None
        acc = [empty_cl(shape1, dev) for _ in range(3)] if need_w else None
        wg = _Wgrad(3, V, D, H, W, 16, 16, dev, he, bf16=True) if need_w else None     # (one scratch: the launches are in order)
        sw = _SideWgrad(dev, need_w)
        if sw.on:
            sw.begin(gwb, zz, UP, RP, CA, RH, HS, wg.scratch, *acc)

        def weight_grads(ci, lo, hi):                             # of steps lo .. hi-1 (their gate gradients are final) + their share of the sums
            j = slice(lo - 1, hi - 1)
            for k, (gp, xh) in enumerate(((UP, HS), (RP, HS), (CA, RH))):
                for q, x in enumerate((zz[lo:hi], xh[j])):
                    wg(x, gp[j], gwb[ci, k, q])
                launch('lf_sum_views_bf16', gp[j], acc[k], n, hi - lo, int(ci > 0))
        for ci, (lo, hi) in enumerate(chunks):
            for i in range(hi - 1, lo - 1, -1):
                j, gnext = slice(i - 1, i), gbuf[i & 1]
                h = HS[j]
                launch('lf_gru_train_stage_b_bwd', g, h, UP[j], CA[j], gh1, UP[j], CA[j], None, None, n, 1)
                ring_multi(CA[j], _one(pk.o.state.t), he, [(RP[j], RP[j], True)], extra=_lib.LF_RING_EX_ABWD, e0=h, e1=gh1, o2=gh12)
                ring_multi(UP[j], _one(pk.u.state.t), he, [(gnext, gh12, False)])
                ring_multi(RP[j], _one(pk.r.state.t), he, [(gnext, gnext, False)])
                g = gnext
            if need_w:                                            # the gate gradients of the chunk's steps are complete
                sw.run(functools.partial(weight_grads, ci, lo, hi))
        if need_z:                                                # the views' gradients, from the stored gate gradients of all steps
            gzs = gz[1:]
            ring_multi(CA, _one(pk.o.z.t), he, [(gzs, None, True)])
            ring_multi(UP, _one(pk.u.z.t), he, [(gzs, gzs, False)])
            ring_multi(RP, _one(pk.r.z.t), he, [(gzs, gzs, False)])
        sw.join()
        if self.z32:
            gz = gz.float()
        return gz, g, gwb, acc


class _GruFuse(torch.autograd.Function):
    """GRUFuser.forward for 16-channel volumes as ONE autograd node (recon/fusion.py:188-197 over modules/gru.py:30-43): the
    recurrence h_i = cell(cat(z_i, coords), h_{i-1}), h_0 = z_0, forward and backward sequenced explicitly.  Compared with the
    per-gate autograd functions (_Conv3x3Sum16 / _GruGates / _GruBlend) this removes every ATen gradient accumulation over full
    volumes (the data gradients of a step chain through the addend form of the convolution, the gate gradients' sums over the
    views are kept by the kernels), the sigmoid outputs are recomputed instead of stored, and under the bf16 autocast policy the
    tensors that only half-precision convolutions produce / consume (gate pre-activations, h*r, candidate, gate gradients) live
    in bf16 storage.  z: (1,V,16,D,H,W) with dense channels-last views.  Returns h_V (1,16,D,H,W)."""

    @staticmethod
    def forward(ctx, z, c16, wu, bu, wr, br, wo, bo):
        B, V = z.shape[0], z.shape[1]
        assert B == 1 and z.shape[2] == 16 and z.is_cuda and z.dtype in (torch.float32, torch.bfloat16)
        zz = _dense_views(z)                                      # (V,16,D,H,W) channels-last, fp32 or bf16 storage
        ac = ops.AUTOCAST is not None
        if not ac:
            zz = _f32(zz)                                         # (a bf16-stored stack fused OUTSIDE the policy: the fp32 kernels read 64 B records)
        he = he_constant(wu)
        pk = _Gates(*(_gate_packs(w, ac) for w in (wu, wr, wo)))
        base = [_gru_conv(ac, he, c16, g.coords.fwd, bias=(b.detach() if b is not None else None)) for g, b in zip(pk, (bu, br, bo))]
        ctx.rec = (_RingRecurrence if _ring_route(ac, V, *zz.shape[2:]) else _StepRecurrence)(ac, he, pk)
        out, zz = ctx.rec.forward(zz, base)
        ctx.save_for_backward(zz, c16, wu, wr, wo)
        ctx.zshape, ctx.has_bias = tuple(z.shape), tuple(b is not None for b in (bu, br, bo))
        return out

    @staticmethod
    def backward(ctx, g):
        zz, c16, wu, wr, wo = ctx.saved_tensors
        need_z = ctx.needs_input_grad[0]
        need_w = any(ctx.needs_input_grad[i] for i in (2, 3, 4, 5, 6, 7))
        gz, g_seed, gwb, acc = ctx.rec.backward(cl(g.reshape((1,) + tuple(zz.shape[1:]))), zz, need_z, need_w)
        if gz is not None:
            gz[0:1].copy_(g_seed)                                 # (h_0 = view 0)
        outs = [gz.view(ctx.zshape) if need_z else None, None]
        outs += _gru_weight_grads(ctx, gwb, acc, c16, (wu, wr, wo), ctx.rec.he, ctx.rec.ac) if need_w else [None] * 6
        return tuple(outs)


def gru_fuse(z, c16, cell):
    """See _GruFuse.  `cell`: the ConvGRUCell (three EqualizedConv3d gates over 16 + 3 + 16 input channels)."""
    gs = (cell.update_gate, cell.reset_gate, cell.out_gate)
    return _GruFuse.apply(z, c16, gs[0].module.weight, gs[0].bias, gs[1].module.weight, gs[1].bias, gs[2].module.weight, gs[2].bias)
