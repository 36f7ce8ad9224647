"""Tape ops of the TransUNet path (R50 hybrid ResNetV2 + ViT encoder + CUP decoder) on libunetmi kernels.

Extends umi/graph.py's `Tape`.  Token tensors [B, N, C] are carried as NHWC [B, 1, N, C] so that `nn.Linear` is a
1x1 convolution on the same kernels.  Values produced here are stored *activated* (plain `Act`, tx = None); only the
decoder's conv+BatchNorm+ReLU layers keep the lazy consumer-side transform of the U-Net path.

Reference semantics (TransUnet/): StdConv2d resnet_skip.py:18-25, PreActBottleneck :38-74, ResNetV2 :112-160,
Embeddings vit_seg_modeling.py:122-165, Attention :50-94, Mlp :97-119, Block :168-187, DecoderBlock :284-315.
"""
import ctypes
import os

import torch

from . import lib as L
from . import ops, ops_tu
from .graph import Act, Tape, _wants_grad


def _no_linear_fusion():
    return os.environ.get("UMI_NO_LINEAR_FUSION") == "1"          # A/B knob, read per call


def _no_wgrad_group():
    return os.environ.get("UMI_NO_WGRAD_GROUP") == "1"           # A/B knob, read per call


# ---- grouped launches of the deferred kinds (umi/deferred.py): items as recorded by the ops below ---------------------------
def _wgrad_single(key, item, tape):
    x, dy, gw = item
    ops.conv_wgrad(x, None, dy, None, gw, *key[-2:], 1, tape.inv, 1, 1, 1, 0, flags=tape._fk(1, 1, 1, 0, x.shape[3], dy.shape[3]))


def _norm_rows_group(rows, items, tape):
    parts, dgs, dbs = zip(*items)
    ops_tu.gn_param_grads_group(parts, rows, dgs, dbs, tape.inv)


def _wstd_group(_, items, tape):
    ents, flat = [e for e, _ in items], items[0][1]
    slots = [tape.grad_sink.buffer_for(e.w()) for e in ents] if tape.grad_sink is not None else None
    tape.pack_cache.wstd_bwd(ents, flat[0], flat[1], slots)


class TUTape(Tape):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.attn_flags = 0               # compute_dtype "fp32_mfma_attn": lib.UMI_ATTN_F32_MFMA, passed to the attention calls
        self._attn_seed_dev = None        # this forward's snapshot of the device step counter (_attn_kw)
        d = self.deferred
        d.marks = True          # fills stay deferred under a gradient sink: flush_mark runs them group by group of layers
        # weight gradients of the token linears, run per SHAPE: one launch for the twelve encoder layers' fc1 weights, one for
        # fc2, ... (umi_conv_wgrad_group; one layer at a time these GEMMs took a 7-9-way split-K whose slabs cost more than the
        # GEMM).  Their bias gradients (column sums of the same dy) ride along.  Items (dy, gb) and (x, dy, gw).
        d.register("colsum", lambda _, items, tape: ops.colsum_group(*zip(*items), tape.inv),
                   each=lambda _, item, tape: ops.colsum(*item, tape.inv))
        d.register("wgrad_group", lambda key, items, tape: ops.conv_wgrad_group(*zip(*items), *key[-2:], tape.inv),
                   each=_wgrad_single, on=lambda tape: not _no_wgrad_group())
        # dgamma / dbeta of the GroupNorm and LayerNorm layers, summed from their rows: one launch per row count
        d.register("norm_rows", _norm_rows_group)
        # StdConv2d standardisation backward of every conv that holds a slot (_wstd_slot): one umi_wstd_bwd_multi launch
        d.register("wstd", _wstd_group)

    # gradients of a value with several consumers are summed by a libunetmi kernel (no torch arithmetic)
    def _give(self, act, g):
        if act.parts is None and act.needs_grad and act.grad is not None:
            act.gives += 1
            if self.deferred.held(act.grad):                # another reader of this buffer is still to come: a deferred
                tgt = torch.empty_like(act.grad)               # weight gradient, or the other addend of a residual add
                ops_tu.add(act.grad, g, tgt)
                act.grad = tgt
                return
            ops_tu.add(act.grad, g, act.grad)
            return
        super()._give(act, g)

    def _accumulate_target(self, act, src, R, S, stride, pad):
        if act.grad is not None and self.deferred.held(act.grad):
            return None                                        # read-only buffer (see _give)
        return super()._accumulate_target(act, src, R, S, stride, pad)

    def _defer_wgrad(self, x, tx, dy, gw, s_co, s_ci):
        """Weight gradient of a token linear: joins its shape's grouped launch (dy stays read-only until then)?"""
        if tx is not None or self.dtype != torch.float16:
            return False
        key = (tuple(x.shape), x.stride(), tuple(dy.shape), dy.stride(), s_co, s_ci)
        return self.deferred.defer("wgrad_group", key, (x, dy, gw), fills=(gw,), reads=(dy,))

    def _defer_colsum(self, dy, gb):
        """Bias gradient = column sums of dy: with the weight gradient deferred, dy is alive until the end of the pass anyway."""
        return self.deferred.held(dy) and self.deferred.defer("colsum", (tuple(dy.shape), dy.stride()), (dy, gb), fills=(gb,))

    # ---- convolution with weight standardisation (no bias), output stored raw == activated -----------------------
    def std_conv(self, a: Act, conv):
        w = conv.weight
        Co, Ci, R, S = w.shape
        stride, pad = conv.stride[0], conv.padding[0]
        N, H, W, Ca = a.shape
        assert Ca == Ci
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        out = self.alloc(N, Ho, Wo, Co, device=a.raw.device)
        c = self.pack_cache
        ent = None
        if c is not None and isinstance(w, torch.nn.Parameter) and w.dtype == torch.float32 and w.is_contiguous():
            # standardised weights and their kernel layouts come from the model's cache: refreshed for all 52 convs of the
            # hybrid by two launches at the start of the step (PackCache.refresh) instead of three launches per conv
            ent = c.wstd(w, 1e-5)
            ws, rstd = ent.ws, ent.rstd

            def packed(kind):
                return lambda lay: c.get(kind, ws, self.dtype, bool(lay))
        else:
            ws, rstd = ops_tu.wstd_fwd(w, 1e-5)

            def packed(kind):
                return lambda lay: ops.PACKERS[kind](ws, self.dtype, k8=bool(lay))
        # (only the mode that opts the pointwise kernels in puts its flags on the standardised convolutions, 3x3 ones included)
        fk = self._fk if self.conv1x1_flags else (lambda *_: 0)
        ops.conv_fwd(a.raw, a.tx, packed("conv_fwd"), None, out, R, S, stride, pad, flags=fk(R, S, stride, pad, Ci, Co))
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                slot = self._wstd_slot(ent, w) if ent is not None else None
                gws = slot[0] if slot is not None else torch.empty_like(ws)
                ops.conv_wgrad(a.raw, a.tx, o.grad, None, gws, Ci * R * S, R * S, 1, self.inv, R, S, stride, pad,
                               flags=fk(R, S, stride, pad, Ci, Co),
                               defer=self.deferred.open("wgrad_reduce") if slot is not None else None)
                # with a slot the standardisation's backward runs once for all convs at the end of the backward pass
                self._set_pgrad(w, slot[1] if slot is not None else ops_tu.wstd_bwd(ws, rstd, gws))
                if _wants_grad(a):
                    dx = self.alloc(N, H, W, Ci, device=out.device)
                    if stride == 1:
                        ops.conv_fwd(o.grad, None, packed("conv_dgrad"), None, dx, R, S, 1, R - 1 - pad,
                                     flags=fk(R, S, 1, R - 1 - pad, Co, Ci))
                    else:
                        self._strided_dgrad(o.grad, packed("conv_dgrad_strided"), dx, R, S, stride, pad)
                    self._give(a, dx)
            self.steps.append(bwd)
        return o

    def _wstd_slot(self, ent, w):
        """(gradient w.r.t. the standardised weight, parameter gradient) views of this conv in two flat per-step buffers; the
        second is filled by ONE umi_wstd_bwd_multi launch at the next flush (under a gradient sink it IS the parameter's bucket
        slot).  None where that deferral is not safe: a conv used twice has ONE slot (its second gradient is computed at once and
        added after the flush, Tape._set_pgrad)."""
        pend = self.deferred.open("wstd")          # (ent, flat buffers) of the convs that hold a slot
        if id(w) in self.param_grads or any(e is ent for e, _ in pend):
            return None
        sink_slot = self.grad_sink.buffer_for(w) if self.grad_sink is not None else None
        if self.grad_sink is not None and sink_slot is None:
            return None
        if pend:
            flat = pend[-1][1]
        else:
            n = self.pack_cache.wstd_total
            flat = (torch.empty(n, dtype=torch.float32, device=w.device),
                    torch.empty(n, dtype=torch.float32, device=w.device) if self.grad_sink is None else None)
        gws = flat[0][ent.off:ent.off + w.numel()].view(w.shape)
        # (under a sink the launch writes the parameter gradient straight into the bucket slot)
        gw = sink_slot if sink_slot is not None else flat[1][ent.off:ent.off + w.numel()].view(w.shape)
        self.deferred.defer("wstd", None, (ent, flat), fills=(gw,))
        return gws, gw

    def flush_mark(self):
        """Marks a point of the forward pass: when the backward pass comes back to it, every deferred gradient fill recorded so far
        runs.  Without a gradient sink this does nothing (one flush at the end is the fewest launches); under one, the model puts
        a mark between the ResNet hybrid and the ViT encoder, so the encoder's ~85 M gradient values (the first two thirds of a
        R50-ViT-B/16's buckets in reduction order) are on the wire while the hybrid's backward pass computes."""
        if self.record and self.grad_sink is not None:
            self.steps.append(self.deferred.flush)

    @staticmethod
    def _strided_dgrad(dy, wpd, dx, R, S, stride, pad):
        N, Hd, Wd, Cd, lddy = ops._nhwc(dy)
        _, Hx, Wx, Cx, lddx = ops._nhwc(dx)
        lay = ctypes.c_int(0)
        L.call("umi_conv_fwd_plan", N, Hd, Wd, Cd, Cx, R, S, stride, pad, lddy, lddx, ops._dt(dy), ops._dt(dx),
               L.CONV_DGRAD_STRIDED, 0, ctypes.addressof(lay), None)
        if callable(wpd):
            wpd = wpd(lay.value)
        elif lay.value != 0:
            raise ValueError("this data gradient takes the MFMA path: pass a callable so the weights get the k8 packing")
        L.call("umi_conv_fwd", dy.data_ptr(), lddy, None, wpd.data_ptr(), None, dx.data_ptr(), lddx, None,
               N, Hd, Wd, Cd, Cx, R, S, stride, pad, Hx, Wx, 0, 0, Hx, Wx, ops._dt(dy), ops._dt(dx),
               L.CONV_DGRAD_STRIDED, ops._stream())

    # ---- GroupNorm (+ residual) (+ ReLU) ---------------------------------------------------------------------------
    def group_norm(self, a: Act, gn, relu, residual: Act = None):
        assert a.tx is None and (residual is None or residual.tx is None)
        N, H, W, C = a.shape
        out = self.alloc(N, H, W, C, device=a.raw.device)
        g32, b32 = gn.weight.detach().float(), gn.bias.detach().float()
        mean, rstd = ops_tu.gn_fwd(a.raw, g32, b32, gn.num_groups, gn.eps, relu, residual.raw if residual is not None else None, out)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dx = self.alloc(N, H, W, C, device=out.device)
                dres = self.alloc(N, H, W, C, device=out.device) if (residual is not None and _wants_grad(residual)) else None
                if (self.dtype == torch.float16 and id(gn.weight) not in self.param_grads
                        and id(gn.bias) not in self.param_grads):
                    # dgamma / dbeta of all GroupNorm layers are summed from their per-sample rows at the next flush
                    part = ops_tu.gn_bwd(o.grad, out, a.raw, mean, rstd, g32, gn.num_groups, relu, dx, dres, self.inv,
                                         keep_part=True)
                    dg, db = self._new_pgrad(gn.weight), self._new_pgrad(gn.bias)
                    self.deferred.defer("norm_rows", N, (part, dg, db), fills=(dg, db))
                else:
                    dg, db = ops_tu.gn_bwd(o.grad, out, a.raw, mean, rstd, g32, gn.num_groups, relu, dx, dres, self.inv)
                self._set_pgrad(gn.weight, dg)
                self._set_pgrad(gn.bias, db)
                if dres is not None:
                    self._give(residual, dres)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def pool3s2(self, a: Act):
        N, H, W, C = a.shape
        out = self.alloc(N, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C, device=a.raw.device)
        idx = None
        if self.record and self.dtype == torch.float16 and C % 8 == 0 and a.raw.stride(2) % 8 == 0:
            idx = torch.empty(out.shape, dtype=torch.uint8, device=out.device)      # winning taps, for the backward
        ops_tu.pool3s2_fwd(a.raw, out, idx)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None or not _wants_grad(a):
                    return
                dx = self.alloc(N, H, W, C, device=out.device)
                ops_tu.pool3s2_bwd(o.grad, a.raw, dx, idx)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def pad_to(self, a: Act, size):
        """Zero-padded top-left copy (resnet_skip.py:150-155)."""
        N, H, W, C = a.shape
        if H == size and W == size:
            return a
        out = self.alloc(N, size, size, C, zero=True, device=a.raw.device)
        out[:, :H, :W, :].copy_(a.raw)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is not None:
                    self._give(a, o.grad[:, :H, :W, :].contiguous())
            self.steps.append(bwd)
        return o

    # ---- token ops -----------------------------------------------------------------------------------------------------
    def linear(self, a: Act, weight, bias, _fused=None):
        """nn.Linear ([Co,Ci] weight) or a 1x1 Conv2d ([Co,Ci,1,1] weight) + bias on [B,1,N,Cin] tokens / NHWC maps.
        `_fused(out, packed_weights, bias32) -> bool` (linear_dropout): runs the forward GEMM itself, with an epilogue."""
        Co = weight.shape[0]
        Ci = weight.numel() // Co                        # the flattened fan-in: C * P * P of the pure ViT's [Co, C, P, P] patch weight
        N, H, W, Ca = a.shape
        assert Ca == Ci
        out = self.alloc(N, H, W, Co, device=a.raw.device)
        w4 = weight.detach().float().reshape(Co, Ci, 1, 1)
        # a weight with taps is packed as its [Co, fan-in] matrix; the PARAMETER stays the key of the pack cache and of the sink
        k_fwd, k_dgrad = ("linear_fwd", "linear_dgrad") if weight.dim() == 4 and weight.shape[1] != Ci else ("conv_fwd", "conv_dgrad")
        b32 = bias.detach().float() if bias is not None else None
        # (kernel-layout copies from the model's PackCache when `weight` is a parameter: MLP / out-projection / patch embedding)
        if _fused is None or not _fused(out, self._packer(k_fwd, weight, w4), b32):
            if _fused is not None:
                return None                             # the caller runs the unfused sequence
            ops.conv_fwd(a.raw, a.tx, self._packer(k_fwd, weight, w4), b32, out, 1, 1, 1, 0,
                         flags=self._fk(1, 1, 1, 0, Ci, Co))
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                gw = self._new_pgrad(weight)
                if not self._defer_wgrad(a.raw, a.tx, o.grad, gw, Ci, 1):
                    ops.conv_wgrad(a.raw, a.tx, o.grad, None, gw, Ci, 1, 1, self.inv, 1, 1, 1, 0, flags=self._fk(1, 1, 1, 0, Ci, Co))
                self._set_pgrad(weight, gw)
                if bias is not None:
                    gb = self._new_pgrad(bias)
                    if not self._defer_colsum(o.grad, gb):
                        ops.colsum(o.grad, gb, self.inv)
                    self._set_pgrad(bias, gb)
                if _wants_grad(a):
                    dx = self.alloc(N, H, W, Ci, device=out.device)
                    ops.conv_fwd(o.grad, None, self._packer(k_dgrad, weight, w4), None, dx, 1, 1, 1, 0,
                                 flags=self._fk(1, 1, 1, 0, Co, Ci))
                    self._give(a, dx)
            self.steps.append(bwd)
        return o

    def patch_rows(self, x: torch.Tensor, P):
        """Graph input of the pure ViT: the P x P patches of the contiguous NCHW image as [B, 1, gh * gw, C * P * P] tokens in the
        compute dtype (umi_patch_rows; column order = the flattening of the [hidden, C, P, P] patch weight).  The image takes no
        gradient."""
        if not x.is_cuda:
            raise RuntimeError("unet-torch_amd: the HIP path needs the input on device 'cuda' (MI355X); "
                               "no CPU fallback exists in the product path")
        if x.dtype not in (torch.float32, torch.float16):
            x = x.float()
        x = x.contiguous()
        B, C, H, W = x.shape
        n, K = (H // P) * (W // P), C * P * P
        raw = self.alloc(B, 1, n, K, device=x.device)
        ops_tu.patch_rows(x, P, raw.view(B * n, K))
        a = Act(raw, None, needs_grad=False)
        self._inputs.append(a)
        return a

    def conv1x1_bias(self, a: Act, conv):
        """Patch embedding: Conv2d(k=1) + bias (vit_seg_modeling.py:145-148)."""
        return self.linear(a, conv.weight, conv.bias)

    def layer_norm(self, a: Act, ln):
        N, H, W, C = a.shape
        out = self.alloc(N, H, W, C, device=a.raw.device)
        g32, b32 = ln.weight.detach().float(), ln.bias.detach().float()
        mean, rstd = ops_tu.ln_fwd(a.raw, g32, b32, ln.eps, out)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dx = self.alloc(N, H, W, C, device=out.device)
                if (self.dtype == torch.float16 and id(ln.weight) not in self.param_grads
                        and id(ln.bias) not in self.param_grads):
                    part, rows = ops_tu.ln_bwd(o.grad, a.raw, g32, mean, rstd, dx, self.inv, keep_part=True)
                    dg, db = self._new_pgrad(ln.weight), self._new_pgrad(ln.bias)
                    self.deferred.defer("norm_rows", rows, (part, dg, db), fills=(dg, db))     # summed with the GroupNorm rows
                else:
                    dg, db = ops_tu.ln_bwd(o.grad, a.raw, g32, mean, rstd, dx, self.inv)
                self._set_pgrad(ln.weight, dg)
                self._set_pgrad(ln.bias, db)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def gelu(self, a: Act):
        out = torch.empty_like(a.raw)
        ops_tu.gelu_fwd(a.raw, out)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dx = torch.empty_like(a.raw)
                ops_tu.gelu_bwd(a.raw, o.grad, dx)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def add(self, a: Act, b: Act):
        out = torch.empty_like(a.raw)
        ops_tu.add(a.raw, b.raw, out)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                # both addends receive the same tensor (no copy): it is marked read-only, an accumulation into either
                # addend's gradient then goes to a fresh tensor (_give) instead of in place
                self.deferred.hold(o.grad)
                self._give(a, o.grad)
                self._give(b, o.grad)
            self.steps.append(bwd)
        return o

    def add_position(self, a: Act, pos):
        """tokens + position_embeddings [1, N, C] (vit_seg_modeling.py:163)."""
        B, _, N, C = a.shape
        out = torch.empty_like(a.raw)
        p = pos.detach().reshape(N, C).to(self.dtype).contiguous()
        ops_tu.add_bcast(a.raw, p, out, N)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                gp = torch.empty(N * C, dtype=torch.float32, device=out.device)
                ops.colsum(o.grad.reshape(1, 1, B, N * C), gp, self.inv)
                self._set_pgrad(pos, gp.view_as(pos))
                self._give(a, o.grad)
            self.steps.append(bwd)
        return o

    def linear_dropout(self, a: Act, weight, bias, p, gelu=False, add: Act = None):
        """dropout(gelu?(linear(a))) + add? with the elementwise tail in the GEMM's epilogue (umi_linear_fused; VERDICT round 2,
        item 4: fc1 = bias + GELU + dropout with the mask byte written by the epilogue, fc2 / attention projection = bias +
        dropout + residual).  Values, masks and the recorded backward are those of dropout(linear(a), p, gelu, add): the
        forward just costs one launch and one pass over the activation less."""
        plain = not self.training or p <= 0.0
        if (plain or self.dtype != torch.float16 or a.tx is not None or (add is not None and add.tx is not None)
                or not (gelu or add is not None) or _no_linear_fusion()):
            return self.dropout(self.linear(a, weight, bias), p, gelu=gelu, add=add)
        N, H, W, _ = a.shape
        Co = weight.shape[0]
        mask = torch.empty(N * H * W * Co, dtype=torch.uint8, device=a.raw.device)
        act = self.alloc(N, H, W, Co, device=a.raw.device) if gelu else None
        self._drop_count += 1
        seed = self._seed * 7919 + self._drop_count

        def fused(out, packed, b32):
            lay, _ = ops.conv_plan(a.raw, out, 1, 1, 1, 0, has_bias=b32 is not None)
            if not lay:
                return False
            return ops_tu.linear_fused(a.raw, packed(lay), b32, out, 1 if gelu else 2, p, seed, self._seed_dev, mask,
                                       aux=add.raw if (add is not None and not gelu) else None, y2=act)
        if gelu and add is not None:                     # (no such block in the reference: GELU and residual never share a linear)
            self._drop_count -= 1
            return self.dropout(self.linear(a, weight, bias), p, gelu=gelu, add=add)
        lin = self.linear(a, weight, bias, _fused=fused)
        if lin is None:
            self._drop_count -= 1
            return self.dropout(self.linear(a, weight, bias), p, gelu=gelu, add=add)
        # epi 1: `lin` holds the pre-activation, `act` the dropped-out GELU; epi 2: `lin`'s buffer holds dropout(.) + add, the
        # pre-dropout values are not kept (the backward needs the mask only)
        o = Act(act if gelu else lin.raw, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dx = torch.empty_like(lin.raw)
                if gelu:
                    if not ops_tu.dropout_fused(o.grad, dx, mask, True, p, 0, None, lin.raw, True):
                        raise RuntimeError("umi_dropout_fused refused the GELU + dropout backward")
                else:
                    ops_tu.dropout(o.grad, dx, mask, True, p, 0)
                if add is not None:
                    self.deferred.hold(o.grad)
                    self._give(add, o.grad)
                self._give(lin, dx)
            self.steps.append(bwd)
        return o

    def dropout(self, a: Act, p, gelu=False, add: Act = None):
        """Dropout(p), optionally with the GELU before it and / or a residual add after it in the same kernel:
        dropout(gelu(a)) + add  (reference Mlp.forward vit_seg_modeling.py:113-119, Block.forward :177-187)."""
        if not self.training or p <= 0.0:
            o = self.gelu(a) if gelu else a
            return self.add(o, add) if add is not None else o
        out = torch.empty_like(a.raw)
        mask = torch.empty(a.raw.numel(), dtype=torch.uint8, device=a.raw.device)
        self._drop_count += 1
        seed = self._seed * 7919 + self._drop_count
        if gelu or add is not None:
            if not (a.tx is None and (add is None or add.tx is None) and
                    ops_tu.dropout_fused(a.raw, out, mask, False, p, seed, self._seed_dev, add.raw if add is not None else None, gelu)):
                self._drop_count -= 1                  # unfused: the same ops one after the other
                o = self.dropout(self.gelu(a) if gelu else a, p)
                return self.add(o, add) if add is not None else o
        else:
            ops_tu.dropout(a.raw, out, mask, False, p, seed, seed_dev=self._seed_dev)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dx = torch.empty_like(a.raw)
                if gelu:
                    if not ops_tu.dropout_fused(o.grad, dx, mask, True, p, 0, None, a.raw, True):     # never inside an assert:
                        raise RuntimeError("umi_dropout_fused refused the GELU + dropout backward")   # `python -O` drops those
                else:
                    ops_tu.dropout(o.grad, dx, mask, True, p, 0)
                if add is not None:                    # the residual branch receives the same tensor (read-only, see add())
                    self.deferred.hold(o.grad)
                    self._give(add, o.grad)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def _attn_kw(self, p=0.0):
        """The attention calls' keywords: none without a flag and without dropout, so that such a tape calls ops_tu.attn_fwd /
        attn_bwd exactly as before (positional arguments only).

        Attention-probability dropout (training, p > 0) stores no mask: forward, dQ and dK/dV kernels each regenerate it from
        (seed, device counter), so the backward call gets the SAME dictionary.  The site takes its seed like the tape's other
        dropout sites (`_drop_count` advances once per site in forward order; untouched for p = 0 or in eval mode).  The other
        sites keep their mask bytes and do not care that dropout_seeds advances the device counter on every training forward;
        a regenerating site does (forward A, forward B, backward A would rebuild A's mask with B's counter), so the tape
        snapshots the counter ONCE per forward into a 4-byte device scalar of its own -- one device copy, capturable, made only
        when an attention site drops -- and every layer's forward and backward read that snapshot."""
        kw = {"flags": self.attn_flags} if self.attn_flags else {}
        if not self.training or p <= 0.0:
            return kw
        if self._seed_dev is not None and self._attn_seed_dev is None:
            self._attn_seed_dev = self._seed_dev.clone()
        self._drop_count += 1
        kw.update(p=float(p), seed=self._seed * 7919 + self._drop_count, seed_dev=self._attn_seed_dev)
        return kw

    def attention(self, q: Act, k: Act, v: Act, heads, p=0.0):
        out = torch.empty_like(q.raw)
        kw = self._attn_kw(p)
        lse = ops_tu.attn_fwd(q.raw, k.raw, v.raw, out, heads, **kw)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dq, dk, dv = torch.empty_like(q.raw), torch.empty_like(q.raw), torch.empty_like(q.raw)
                ops_tu.attn_bwd(q.raw, k.raw, v.raw, out, o.grad, lse, dq, dk, dv, heads, **kw)
                self._give(q, dq)
                self._give(k, dk)
                self._give(v, dv)
            self.steps.append(bwd)
        return o

    def qkv_attention(self, a: Act, query, key, value, heads, p=0.0):
        """softmax(QK^T/sqrt(d))V with the three projections of `a` (reference Attention.forward, vit_seg_modeling.py:73-91)
        run as ONE GEMM of width 3C: q/k/v are channel slices of one buffer, so the data gradient is one GEMM with
        K = 3C (no summing of three partial gradients) and the three weight / bias gradients come out of one launch each.
        The modules stay separate `nn.Linear`s (reference state_dict keys); their weights are concatenated per step."""
        N, H, W, C = a.shape
        mods = (query, key, value)
        c = self.pack_cache
        if c is not None and all(isinstance(t_, torch.nn.Parameter) and t_.dtype == torch.float32 and t_.is_contiguous()
                                 for m in mods for t_ in (m.weight, m.bias)):
            # the concatenated operands live in the model's cache, each projection packed into its slice by the step's one
            # pack launch (no torch.cat, no per-layer pack launches)
            wts = [m.weight for m in mods]
            bcat = c.get_cat("bias", [m.bias for m in mods], torch.float32, False)

            def packed(kind):
                return lambda lay: c.get_cat(kind, wts, self.dtype, bool(lay))
        else:
            wcat = torch.cat([m.weight.detach().float() for m in mods], 0).reshape(3 * C, C, 1, 1)
            bcat = torch.cat([m.bias.detach().float() for m in mods], 0)

            def packed(kind):
                return lambda lay: ops.PACKERS[kind](wcat, self.dtype, k8=bool(lay))
        qkv = self.alloc(N, H, W, 3 * C, device=a.raw.device)
        ops.conv_fwd(a.raw, a.tx, packed("conv_fwd"), bcat, qkv, 1, 1, 1, 0, flags=self._fk(1, 1, 1, 0, C, 3 * C))
        q, k, v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
        out = self.alloc(N, H, W, C, device=a.raw.device)
        kw = self._attn_kw(p)                           # (with p > 0: this site's seed and the counter snapshot, see there)
        lse = ops_tu.attn_fwd(q, k, v, out, heads, **kw)
        o = Act(out, None)
        if self.record:
            def bwd():
                if o.grad is None:
                    return
                dqkv = self.alloc(N, H, W, 3 * C, device=out.device)
                ops_tu.attn_bwd(q, k, v, out, o.grad, lse, *(dqkv[..., i * C:(i + 1) * C] for i in range(3)), heads, **kw)
                if self.grad_sink is not None:
                    # three items of the grouped launches, each writing its own bucket slot (the fused [3C, C] gradient would
                    # have to be copied into the three slots afterwards)
                    for i, m in enumerate(mods):
                        d_i = dqkv[..., i * C:(i + 1) * C]
                        gw = self._new_pgrad(m.weight)
                        if not self._defer_wgrad(a.raw, a.tx, d_i, gw, C, 1):
                            ops.conv_wgrad(a.raw, a.tx, d_i, None, gw, C, 1, 1, self.inv, 1, 1, 1, 0, flags=self._fk(1, 1, 1, 0, C, C))
                        self._set_pgrad(m.weight, gw)
                        gb = self._new_pgrad(m.bias)
                        if not self._defer_colsum(d_i, gb):
                            ops.colsum(d_i, gb, self.inv)
                        self._set_pgrad(m.bias, gb)
                else:
                    gw = torch.empty(3 * C, C, dtype=torch.float32, device=out.device)
                    if not self._defer_wgrad(a.raw, a.tx, dqkv, gw, C, 1):
                        ops.conv_wgrad(a.raw, a.tx, dqkv, None, gw, C, 1, 1, self.inv, 1, 1, 1, 0,
                                       flags=self._fk(1, 1, 1, 0, C, 3 * C))
                    gb = torch.empty(3 * C, dtype=torch.float32, device=out.device)
                    if not self._defer_colsum(dqkv, gb):
                        ops.colsum(dqkv, gb, self.inv)
                    for i, m in enumerate(mods):
                        self._set_pgrad(m.weight, gw[i * C:(i + 1) * C])
                        self._set_pgrad(m.bias, gb[i * C:(i + 1) * C])
                if _wants_grad(a):
                    dx = self.alloc(N, H, W, C, device=out.device)
                    ops.conv_fwd(dqkv, None, packed("conv_dgrad"), None, dx, 1, 1, 1, 0, flags=self._fk(1, 1, 1, 0, 3 * C, C))
                    self._give(a, dx)
            self.steps.append(bwd)
        return o

    # ---- decoder -------------------------------------------------------------------------------------------------------
    def bilinear2x_into(self, a: Act, dest):
        """UpsamplingBilinear2d(x2, align_corners=True) of the *activated* `a`, written into `dest` (a channel slice)."""
        N, H, W, C = a.shape
        assert tuple(dest.shape) == (N, 2 * H, 2 * W, C)
        ops_tu.bilinear2x(a.raw, dest, False, a.tx)
        o = Act(dest, None)
        if self.record:
            def bwd():
                if o.grad is None or not _wants_grad(a):
                    return
                dx = self.alloc(N, H, W, C, device=dest.device)
                ops_tu.bilinear2x(o.grad, dx, True)
                self._give(a, dx)
            self.steps.append(bwd)
        return o

    def copy_into(self, a: Act, dest):
        """Place a stored-activated tensor into a channel slice of a concat buffer."""
        assert a.tx is None
        dest.copy_(a.raw)
        o = Act(dest, None)
        if self.record:
            def bwd():
                if o.grad is not None:
                    self._give(a, o.grad.contiguous())
            self.steps.append(bwd)
        return o

    def tokens_to_map(self, a: Act, h, w):
        """[B,1,N,C] tokens -> [B,h,w,C] feature map: a free view in NHWC (vit_seg_modeling.py:356-359)."""
        B, _, N, C = a.shape
        o = Act(a.raw.view(B, h, w, C), None)
        if self.record:
            def bwd():
                if o.grad is not None:
                    self._give(a, o.grad.reshape(B, 1, N, C))
            self.steps.append(bwd)
        return o

    def map_to_tokens(self, a: Act):
        N, H, W, C = a.shape
        o = Act(a.raw.view(N, 1, H * W, C), None)
        if self.record:
            def bwd():
                if o.grad is not None:
                    self._give(a, o.grad.reshape(N, H, W, C))
            self.steps.append(bwd)
        return o
