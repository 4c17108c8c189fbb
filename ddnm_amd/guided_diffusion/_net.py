"""Host scaffold shared by the three networks (models.Model, unet.UNetModel, classifier.EncoderUNetModel).

Nothing here computes: these are the pieces of the Python layer that drive the HIP kernels of ddnm_amd/ops.py and that
were the same, launch for launch, in more than one network:

  * `HostNet`     -- the `nn.Module`-like surface every network offers (`to`, `eval`, `parameters`);
  * `GraphedNet`  -- what the two noise predictors (`Model`, `UNetModel`) share around their eager forward: the per-stream
    GroupNorm workspace and the dispatch ladder of `forward` (chunks -> captured graph -> auto graph -> eager);
  * `ADMNet`      -- what the two ADM-family networks (`UNetModel`, `EncoderUNetModel`; in the reference they share
    ResBlock, AttentionBlock, the time embedding and the encoder constructor of guided_diffusion/unet.py) share: the
    encoder block plan, the FiLM offset table, the per-layer shape table, the embedding head, the fp32 attention
    launches, and the 3x3 / attention blocks of the fp16-activation path.

What differs in substance stays with its network: `load_state_dict`, the ResBlocks (tape, shared prefix, `fin=`),
`_gn`, the classifier's workspace and all backward code, and the single-head attention of `Model`.
"""
import math
from collections import OrderedDict

import torch

from .. import ops
from ..graph import GraphedForward


def random_state_dict(shapes, seed):
    """Seeded random weights for a name -> shape table (no checkpoints exist offline): N(0, 1/fan_in) kernels, GN gamma
    near 1."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, shape in shapes.items():
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            sd[name] = torch.randn(shape, generator=g) * fan_in ** -0.5
        elif name.endswith(".weight"):
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            sd[name] = 0.05 * torch.randn(shape, generator=g)
    return sd


class HostNet:
    # ------------------------------------------------------------------ nn.Module-like surface
    def to(self, device):
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())


class GraphedNet(HostNet):
    """A noise predictor called as `forward(x, t[, y])`.  The subclass supplies `_forward_eager(x, t, y)`,
    `max_forward_batch`, `max_ch`, `_max_gn_partials()` and `TWO_STREAMS`."""
    TWO_STREAMS = False            # default of enable_graphs(two_streams=...)
    auto_graph_max_batch = 0
    _graphs = None
    _auto_graphs = None
    _ws = None

    def _reset_host_state(self):
        """New weights: the workspaces are dropped and captured graphs (which replay the old pointers) are stale."""
        self._ws = None
        self._ws_by_stream = {}
        if self._graphs is not None:
            self._graphs.reset()
        self._auto_graphs = None

    def _workspace(self, B):
        """GroupNorm scratch of the current stream (the affine of one GroupNorm is consumed by the next launch on the
        same stream; the two half-batch streams of a captured forward each own one: see ddnm_amd/graph.py)."""
        key = torch.cuda.current_stream().cuda_stream
        ent = self._ws_by_stream.get(key)
        if ent is None or ent[1] < B:
            ent = (ops.GroupNormWorkspace(self.device, B, self.max_ch, B * self._max_gn_partials() * 32 * 2), B)
            self._ws_by_stream[key] = ent
        self._ws = ent[0]
        return self._ws

    def enable_graphs(self, two_streams=None):
        """Replay the forward from a captured hipGraph (one per batch shape): no per-launch host work, and with
        `two_streams` the two halves of the batch run as concurrent branches of the graph (ddnm_amd/graph.py)."""
        self._graphs = GraphedForward(self._forward_eager,
                                      two_streams=self.TWO_STREAMS if two_streams is None else two_streams)
        return self

    def disable_graphs(self):
        self._graphs = None
        return self

    def auto_graphs(self, max_batch=2):
        """Replay forwards of at most `max_batch` images from a captured hipGraph, decided per call (0: never).  The
        reference's shipped configs sample with batch_size 1 (configs/celeba_hq.yml:34-35, configs/imagenet_256.yml:42);
        a forward is ~250-300 launches whose host cost (~15 us each through ctypes) then exceeds their GPU time, and
        `cudnn.benchmark` was the reference's own small-batch lever (main.py:145).  The runner (`Diffusion`) switches
        this on."""
        self.auto_graph_max_batch = int(max_batch)
        self._auto_graphs = None
        return self

    def forward(self, x, t, y=None):
        mb = self.max_forward_batch
        if x.shape[0] > mb:          # more images than one launch can address: micro-batches, concatenated
            return torch.cat([self.forward(x[i:i + mb], t[i:i + mb], None if y is None else y[i:i + mb])
                              for i in range(0, x.shape[0], mb)], 0)
        if self._graphs is not None:
            return self._graphs(x, t, y)
        if x.shape[0] <= self.auto_graph_max_batch:
            if self._auto_graphs is None:
                self._auto_graphs = GraphedForward(self._forward_eager, two_streams=False)
            return self._auto_graphs(x, t, y)
        return self._forward_eager(x, t, y)


def conv3x3_16(w16, cout, x0, x1, gn, silu=True, **kw):
    """3x3 convolution (or data-gradient convolution) of act(concat(x0, x1)) on ddnm_conv16 with the GroupNorm affine +
    swish of `gn` and the concat fused into its loader; images too small for a
    pixel tile (8x8) go through im2col + one GEMM with K = 9*Cin.  `w16`: the fp16 (O,ky,kx,I) pack."""
    t0, t1 = ops.tensor_of(x0), ops.tensor_of(x1)
    B, H, W, _ = t0.shape
    cin = t0.shape[3] + (0 if t1 is None else t1.shape[3])
    ups = kw.get("ups", False)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    if ops.conv16_supported(B, Ho, Wo, cin, cout, 3, ups=ups):
        return ops.conv16(x0, w16, cout, 3, src1=x1, gn=gn, gn_silu=silu, **kw)
    assert not ups and kw.get("skip") is None
    col = ops.im2col16(x0, x1, gn, silu)
    return ops.conv16(col, w16.reshape(w16.shape[0], 1, -1), cout, 1, **kw)


class ADMNet(HostNet):
    """guided_diffusion/unet.py family: block plans are lists of layers ("conv", cin, cout) / ("res", cin, cout, mode
    [, channels of `h` in the concat]) / ("attn", c), named like the reference's state-dict prefixes."""
    output_blocks = ()             # the encoder-only network has none

    def _plan_encoder(self, in_channels, mc, channel_mult, num_res_blocks, attention_resolutions):
        """`input_blocks` and `middle_block` (unet.py:482-565 / :740-823); returns (channels, downsampling factor) at
        the bottom."""
        ch = int(channel_mult[0] * mc)
        self.input_blocks = [[("conv", in_channels, ch)]]
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [("res", ch, int(mult * mc), "")]
                ch = int(mult * mc)
                if ds in attention_resolutions:
                    layers.append(("attn", ch))
                self.input_blocks.append(layers)
            if level != len(channel_mult) - 1:
                self.input_blocks.append([("res", ch, ch, "down")])
                ds *= 2
        self.middle_block = [("res", ch, ch, ""), ("attn", ch), ("res", ch, ch, "")]
        return ch, ds

    def _walk(self):
        for i, layers in enumerate(self.input_blocks):
            yield f"input_blocks.{i}", layers
        yield "middle_block", self.middle_block
        for i, layers in enumerate(self.output_blocks):
            yield f"output_blocks.{i}", layers

    def _plan_film(self):
        # FiLM projection layout: one slice [2*cout] per ResBlock, in execution order
        off, self._film_off = 0, {}
        for prefix, layers in self._walk():
            for j, L in enumerate(layers):
                if L[0] == "res":
                    self._film_off[f"{prefix}.{j}"] = off
                    off += 2 * L[2]
        self.film_total = off

    def _w16(self, key):
        return self.w.get(key + ".f16") if self.use_fp16 else None

    def _layer_shapes(self, s):
        """The per-layer part of `state_dict_shapes`: name -> shape of every block tensor, in walk order."""
        ted = self.time_embed_dim
        for prefix, layers in self._walk():
            for j, L in enumerate(layers):
                n = f"{prefix}.{j}"
                if L[0] == "conv":
                    s[n + ".weight"], s[n + ".bias"] = (L[2], L[1], 3, 3), (L[2],)
                elif L[0] == "res":
                    cin, cout = L[1], L[2]
                    s[n + ".in_layers.0.weight"], s[n + ".in_layers.0.bias"] = (cin,), (cin,)
                    s[n + ".in_layers.2.weight"], s[n + ".in_layers.2.bias"] = (cout, cin, 3, 3), (cout,)
                    s[n + ".emb_layers.1.weight"], s[n + ".emb_layers.1.bias"] = (2 * cout, ted), (2 * cout,)
                    s[n + ".out_layers.0.weight"], s[n + ".out_layers.0.bias"] = (cout,), (cout,)
                    s[n + ".out_layers.3.weight"], s[n + ".out_layers.3.bias"] = (cout, cout, 3, 3), (cout,)
                    if cin != cout:
                        s[n + ".skip_connection.weight"], s[n + ".skip_connection.bias"] = (cout, cin, 1, 1), (cout,)
                else:
                    c = L[1]
                    s[n + ".norm.weight"], s[n + ".norm.bias"] = (c,), (c,)
                    s[n + ".qkv.weight"], s[n + ".qkv.bias"] = (3 * c, c, 1), (3 * c,)
                    s[n + ".proj_out.weight"], s[n + ".proj_out.bias"] = (c, c, 1), (c,)

    def _time_embed(self, timesteps, device):
        """timestep_embedding -> `time_embed` (unet.py:649 / :880)."""
        w = self.w
        t = timesteps.to(device=device, dtype=torch.float32).contiguous()
        emb = ops.timestep_embedding(t, w["time.freq"], order=1)
        emb = ops.linear(emb, w["time_embed.0.weight"], w["time_embed.0.bias"])
        return ops.linear(emb, w["time_embed.2.weight"], w["time_embed.2.bias"], silu_in=True)

    def _film_all(self, emb):
        """All `emb_layers` Linears of the network in one launch: rows [scale | shift] per ResBlock at `_film_off`."""
        return ops.linear(emb, self.w["film_cat.weight"], self.w["film_cat.bias"], silu_in=True)

    def _attn32(self, n, x, gn, hc):
        """AttentionBlock on fp32 tensors after its GroupNorm affine `gn`: qkv conv, QK^T, softmax, PV, proj conv with the
        residual; heads of `hc` channels are strided views of the fused qkv tensor (QKVAttentionLegacy, unet.py:339-354).
        Returns (output `Act`, qkv, probabilities) -- the last two are what a backward pass keeps."""
        w = self.w
        B, H, W, C = x.t.shape
        T = H * W
        nh = C // hc
        qkv = ops.conv2d(x, w[n + ".qkv.weight"], 3 * C, 1, gn=gn, gn_silu=False, bias=w[n + ".qkv.bias"],
                         weight_f16=self._w16(n + ".qkv.weight"))
        flat = qkv.view(-1)
        S = torch.empty(B * nh, T, T, dtype=torch.float32, device=qkv.device)
        ops.bgemm(flat, flat[hc:], S, T, T, hc, lda=3 * C, ldb=3 * C, ldc=T, transb=True, batch=B * nh, inner=nh,
                  sA=(T * 3 * C, 3 * hc), sB=(T * 3 * C, 3 * hc), sC=(nh * T * T, T * T))
        ops.softmax_rows_(S, B * nh * T, T, T, 1.0 / math.sqrt(hc))      # (q*s).(k*s), s = hc^-1/4
        o = torch.empty(B, H, W, C, dtype=torch.float32, device=qkv.device)
        ops.bgemm(S, flat[2 * hc:], o, T, hc, T, lda=T, ldb=3 * C, ldc=C, transb=False, batch=B * nh, inner=nh,
                  sA=(nh * T * T, T * T), sB=(T * 3 * C, 3 * hc), sC=(T * C, hc))
        out = ops.conv2d(o, w[n + ".proj_out.weight"], C, 1, bias=w[n + ".proj_out.bias"], res=x, emit_stats=True,
                         weight_f16=self._w16(n + ".proj_out.weight"))
        return out, qkv, S

    def _attn_block16(self, n, x, gn, hc, w_qkv, w_proj, lse=None):
        """AttentionBlock of the fp16-activation path after its GroupNorm affine `gn`: normalised operand, qkv GEMM, fused
        attention (`lse`: see ops.attn16), proj GEMM with the residual.  `w_qkv` / `w_proj`: the fp16 packs.
        Returns (output `Act`, qkv, attention output) -- the last two are what a backward pass keeps."""
        w = self.w
        C = x.t.shape[3]
        if hc != 64:
            raise NotImplementedError("the fused attention kernels are built for 64-channel heads (all DDNM configs)")
        a = ops.gn_apply16(x, None, gn, False)
        qkv = ops.conv16(a, w_qkv, 3 * C, 1, bias=w[n + ".qkv.bias"], emit_stats=False).t
        o = ops.attn16(qkv, C, lse=lse)
        return ops.conv16(o, w_proj, C, 1, bias=w[n + ".proj_out.bias"], res=x), qkv, o
