"""Driver for the raw encoder C ABI (include/siglip_hip.h), used by tests/test_abi_contract_gpu.py and
tests/test_abi_contract_host.py.  A plain module: no tests, no fixtures.  It binds the entry points an integrator binds
 through ``pkg.lib`` and never goes through ``SiglipVisionModelHIP``.

* ``Arena``   one uint8 allocation of guard + payload + guard bytes, all filled with one byte value first.  The payload is
              exactly as large as the ABI said it has to be, so a write past it lands in the trailing guard (memory the test
              owns) and is seen by ``guards_intact()``; a read of a byte nobody wrote returns the fill, and 0xFF bytes read
              as NaN in fp32 / bf16 / fp16 and as the NaN scale of an MX block, so it poisons whatever is computed from it.
              Outputs and gradient destinations are Arenas too (their guards are the sentinel rows before and after).
* ``Session`` a context (sgl_create_ex), fp32 masters on the GPU, the sgl_weights struct, sizes, prepare / forward /
              backward through either entry-point family.  Status codes are returned, never raised.
* ``Run``     the arenas and outputs of one (B, H, W, train) geometry.
* ``Grads``   gradient destinations: which pointers are NULL, whether q/k/v weight gradients are one back-to-back buffer,
              the accumulate flag and the prior contents.
* ``Reference`` the CPU oracle (oracle.vision_forward, fp32, autograd) on the same seeded weights with the probe loss,
              cached per (config, shape, ...), and the project's gradient bars.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import torch

GUARD = 64 * 1024          # bytes before and after every payload; a multiple of 256 keeps the payload's alignment
MODES = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "mxfp8": 5}
TRAIN_MODES = ["fp32", "bf16x3", "bf16", "fp16"]
OPERAND = {"fp32": torch.float32, "bf16x3": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16,
           "mxfp8": torch.bfloat16}
OK, ERR_BAD_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_HIP, ERR_NULL = 0, -1, -2, -3, -4, -5

# sgl_weights / sgl_grads field -> HuggingFace state-dict name
GLOBAL_NAMES = {
    "patch_w": "embeddings.patch_embedding.weight", "patch_b": "embeddings.patch_embedding.bias",
    "pos": "embeddings.position_embedding.weight", "post_ln_w": "post_layernorm.weight",
    "post_ln_b": "post_layernorm.bias"}
HEAD_NAMES = {
    "probe": "head.probe", "in_proj_w": "head.attention.in_proj_weight", "in_proj_b": "head.attention.in_proj_bias",
    "out_proj_w": "head.attention.out_proj.weight", "out_proj_b": "head.attention.out_proj.bias",
    "head_ln_w": "head.layernorm.weight", "head_ln_b": "head.layernorm.bias", "head_fc1_w": "head.mlp.fc1.weight",
    "head_fc1_b": "head.mlp.fc1.bias", "head_fc2_w": "head.mlp.fc2.weight", "head_fc2_b": "head.mlp.fc2.bias"}
LAYER_NAMES = {
    "ln1_w": "layer_norm1.weight", "ln1_b": "layer_norm1.bias", "q_w": "self_attn.q_proj.weight",
    "q_b": "self_attn.q_proj.bias", "k_w": "self_attn.k_proj.weight", "k_b": "self_attn.k_proj.bias",
    "v_w": "self_attn.v_proj.weight", "v_b": "self_attn.v_proj.bias", "o_w": "self_attn.out_proj.weight",
    "o_b": "self_attn.out_proj.bias", "ln2_w": "layer_norm2.weight", "ln2_b": "layer_norm2.bias",
    "fc1_w": "mlp.fc1.weight", "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias"}


def layer_name(l, field):
    return f"encoder.layers.{l}.{LAYER_NAMES[field]}"


def stream():
    return torch.cuda.current_stream().cuda_stream


class Arena:
    def __init__(self, nbytes, fill=0x00, device="cuda"):
        self.nbytes, self.fill = int(nbytes), int(fill)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), self.fill, dtype=torch.uint8, device=device)
        assert not self.buf.is_cuda or self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    @property
    def payload(self):
        return self.buf[GUARD:GUARD + self.nbytes]

    def poison(self, fill=None):
        self.payload.fill_(self.fill if fill is None else fill)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.nbytes:] == self.fill).all())

    def untouched(self):
        return bool((self.payload == self.fill).all())

    def f32(self, *shape):
        return self.payload.view(torch.float32).view(*shape)


def make_config(pkg, cfg_name, use_head=1):
    cfg = pkg.get_config(cfg_name)
    return cfg if use_head else dataclasses.replace(cfg, vision_use_head=False)


def sgl_config(pkg, cfg, mode, use_head=1):
    return pkg.lib.SglConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                             cfg.patch_size, cfg.native_grid, cfg.layer_norm_eps, MODES[mode], 1 if use_head else 0)


def weights_struct(pkg, cfg, pointer_of):
    """sgl_weights whose device pointers come from pointer_of(hf_name) (None = NULL).  Returns (struct, layers array)."""
    Lb = pkg.lib
    L = cfg.num_hidden_layers
    layers = (Lb.SglLayerPtrs * max(L, 1))()
    w = Lb.SglWeights()
    w.layers = C.cast(layers, C.POINTER(Lb.SglLayerPtrs))
    for f, n in GLOBAL_NAMES.items():
        setattr(w, f, pointer_of(n))
    for f, n in HEAD_NAMES.items():
        setattr(w, f, pointer_of(n) if cfg.vision_use_head else None)
    for l in range(L):
        for f in LAYER_NAMES:
            setattr(layers[l], f, pointer_of(layer_name(l, f)))
    return w, layers


class Session:
    def __init__(self, pkg, lib, cfg_name, mode, recompute=0, use_head=1, seed=0, device="cuda"):
        self.pkg, self.lib, self.mode, self.recompute, self.use_head = pkg, lib, mode, int(recompute), int(use_head)
        self.cfg_name, self.seed, self.device = cfg_name, seed, device
        self.cfg = make_config(pkg, cfg_name, use_head)
        c = self.cfg
        self.D, self.I, self.Lyr, self.P, self.g0 = (c.hidden_size, c.intermediate_size, c.num_hidden_layers,
                                                     c.patch_size, c.native_grid)
        self.Kp = (3 * self.P * self.P + 63) // 64 * 64
        self.ctx = lib.sgl_create_ex(C.byref(sgl_config(pkg, c, mode, use_head)), self.recompute)
        assert self.ctx, f"sgl_create_ex({cfg_name}, {mode}, recompute={recompute}) returned NULL"
        self.sd = pkg.weights.seeded_state_dict(c, seed=seed)
        self.masters = {k: v.to(device).contiguous() for k, v in self.sd.items()}
        self.w, self._wl = weights_struct(pkg, c, lambda n: self.masters[n].data_ptr())

    def close(self):
        if self.ctx:
            self.lib.sgl_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.close()

    def set_masters(self, sd, only=None):
        """Overwrite master values in place (the struct's pointers stay valid)."""
        for k, v in sd.items():
            if only is None or only(k):
                self.masters[k].copy_(v)

    def sizes(self, B, H, W, train):
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = self.lib.sgl_query_sizes(self.ctx, B, H, W, 1 if train else 0, C.byref(a), C.byref(b), C.byref(c))
        return st, a.value, b.value, c.value

    def geometry(self, B, H, W):
        gh, gw = H // self.P, W // self.P
        return gh, gw, gh * gw, B * gh * gw

    def new_shadow(self, fill=0x00):
        st, sh, _, _ = self.sizes(1, self.P, self.P, False)
        assert st == OK
        return Arena(sh, fill, self.device)

    def prepare(self, shadow, dirty=None, globals_dirty=1, full=False):
        """full: sgl_prepare_weights; otherwise sgl_prepare_weights_dirty(dirty flags or NULL, globals_dirty)."""
        if full:
            return self.lib.sgl_prepare_weights(self.ctx, C.byref(self.w), shadow.ptr, shadow.nbytes, stream())
        flags = None if dirty is None else bytes(bytearray(1 if d else 0 for d in dirty))
        return self.lib.sgl_prepare_weights_dirty(self.ctx, C.byref(self.w), shadow.ptr, shadow.nbytes, flags,
                                                  int(globals_dirty), stream())

    def pixels(self, B, H, W, seed=1):
        return self.pkg.weights.seeded_pixels(B, H, W, seed=seed).to(self.device)

    def patch_operand(self, px, B, H, W):
        """The ready patch-major operand of channels_last == 2: sgl_op_im2col's output in the compute dtype."""
        _, _, _, M = self.geometry(B, H, W)
        out = torch.empty((M, self.Kp), dtype=OPERAND[self.mode], device=self.device)
        dt = MODES["fp32"] if self.mode == "bf16x3" else MODES["bf16"] if self.mode == "mxfp8" else MODES[self.mode]
        st = self.lib.sgl_op_im2col(px.data_ptr(), 0, out.data_ptr(), dt, B, H, W, self.P, self.Kp, stream())
        assert st == OK
        return out

    def forward(self, run, shadow, pixels, kind="contiguous", ex=False, channels_last=0, interp=1, first_trainable=0,
                pooled=True):
        """kind 'contiguous': sgl_forward (sgl_forward_ex when ex) on run.hs_block; 'slots': sgl_forward_slots."""
        lib, r = self.lib, run
        pooled_ptr = r.pooled.ptr if pooled else None
        saved_ptr, saved_n = (r.saved.ptr, r.saved.nbytes) if r.train else (None, 0)
        common = (r.last.ptr, pooled_ptr, saved_ptr, saved_n, r.ws.ptr, r.ws.nbytes)
        head = (self.ctx, C.byref(self.w), shadow.ptr, pixels.data_ptr(), channels_last, r.B, r.H, r.W, int(interp))
        if kind == "slots":
            return lib.sgl_forward_slots(*head, r.slot_table(), *common, int(first_trainable), stream())
        if ex:
            return lib.sgl_forward_ex(*head, r.hs_block.ptr, r.n_slots, *common, int(first_trainable), stream())
        assert first_trainable == 0
        return lib.sgl_forward(*head, r.hs_block.ptr, r.n_slots, *common, stream())

    def backward(self, run, shadow, grads, kind="contiguous", d_last=None, d_pooled=None, d_taps=None,
                 first_trainable=0, train_embeddings=1, interp=1, poison_ws=None):
        """kind 'contiguous': sgl_backward; 'steps': sgl_backward_begin -> sgl_backward_layer -> sgl_backward_embed;
        'slots': sgl_backward_begin_p -> sgl_backward_layer_p -> sgl_backward_embed.  d_taps: list of L+1 tensors / None.
        poison_ws: fill the workspace with this byte first (allowed before sgl_backward_begin)."""
        lib, r, L = self.lib, run, self.Lyr
        if poison_ws is not None:
            r.ws.poison(poison_ws)
        p = lambda t: None if t is None else t.data_ptr()
        taps = [None] * (L + 1) if d_taps is None else list(d_taps)
        tail = (r.saved.ptr, r.saved.nbytes, r.ws.ptr, r.ws.nbytes, stream())
        dims = (r.B, r.H, r.W)
        wsg = (self.ctx, C.byref(self.w), shadow.ptr, C.byref(grads.struct))
        if kind == "contiguous":
            table = None
            if d_taps is not None:
                table = (C.c_void_p * (L + 1))(*[p(t) for t in taps])
            return lib.sgl_backward(*wsg, *dims, int(interp), r.hs_block.ptr, table, p(d_last), p(d_pooled),
                                    int(first_trainable), int(train_embeddings), *tail)
        stop = max(0, 0 if train_embeddings else first_trainable)
        if kind == "steps":
            hs_of = lambda l: r.hs_block.ptr          # the contiguous entry points index the block themselves
            begin, layer = lib.sgl_backward_begin, lib.sgl_backward_layer
        else:
            hs_of = lambda l: r.hidden_ptr(l)
            begin, layer = lib.sgl_backward_begin_p, lib.sgl_backward_layer_p
        st = begin(*wsg, *dims, hs_of(L), p(d_last), p(d_pooled), p(taps[L]), *tail)
        if st != OK:
            return st
        for l in range(L - 1, stop - 1, -1):
            need_dx = 1 if (l > stop or train_embeddings) else 0          # sgl_backward's own rule
            st = layer(*wsg, l, *dims, hs_of(l), p(taps[l]), need_dx, *tail)
            if st != OK:
                return st
        if train_embeddings:
            st = lib.sgl_backward_embed(self.ctx, C.byref(self.w), C.byref(grads.struct), *dims, int(interp), *tail)
        return st


class Run:
    """Arenas and outputs of one geometry, every byte `fill` first.  kind 'contiguous': one [n_slots][M][D] block;
    'slots': L+1 separate buffers."""

    def __init__(self, ses, B, H, W, train, fill=0x00, kind="contiguous", n_slots=None):
        self.ses, self.B, self.H, self.W, self.train, self.fill, self.kind = ses, B, H, W, bool(train), fill, kind
        st, _, saved, ws = ses.sizes(B, H, W, train)
        assert st == OK, f"sgl_query_sizes status {st}"
        self.gh, self.gw, self.N, self.M = ses.geometry(B, H, W)
        dev, L, D = ses.device, ses.Lyr, ses.D
        self.saved = Arena(saved, fill, dev) if train else None
        self.ws = Arena(ws, fill, dev)
        self.n_slots = L + 1 if n_slots is None else n_slots
        self.slot_bytes = self.M * D * 4
        if kind == "contiguous":
            self.hs_block = Arena(self.n_slots * self.slot_bytes, fill, dev)
            self.hs_list = None
        else:
            self.hs_block = None
            self.hs_list = [Arena(self.slot_bytes, fill, dev) for _ in range(L + 1)]
        self.last = Arena(self.slot_bytes, fill, dev)
        self.pooled = Arena(B * D * 4, fill, dev)
        self._table = None

    def slot_table(self):
        self._table = (C.c_void_p * (self.ses.Lyr + 1))(*[a.ptr for a in self.hs_list])
        return self._table

    def hidden_ptr(self, l):
        if self.kind == "contiguous":
            return self.hs_block.ptr + (l % self.n_slots) * self.slot_bytes
        return self.hs_list[l].ptr

    def slot(self, i):
        """Slot i of the contiguous block as an [M, D] tensor."""
        return self.hs_block.f32(self.n_slots, self.M, self.ses.D)[i]

    def hidden(self, l):
        if self.kind == "contiguous":
            return self.slot(l % self.n_slots)
        return self.hs_list[l].f32(self.M, self.ses.D)

    def arenas(self):
        out = [("ws", self.ws), ("last_hidden", self.last), ("pooled", self.pooled)]
        if self.saved is not None:
            out.append(("saved", self.saved))
        if self.hs_block is not None:
            out.append(("hidden_states", self.hs_block))
        else:
            out += [(f"hs_slot{l}", a) for l, a in enumerate(self.hs_list)]
        return out

    def outputs(self, pooled=True):
        """Clones of pooled / last / every hidden state (training layout: slot l = hidden_states[l])."""
        D = self.ses.D
        o = {"last": self.last.f32(self.M, D).clone()}
        if pooled:
            o["pooled"] = self.pooled.f32(self.B, D).clone()
        if self.n_slots == self.ses.Lyr + 1:
            for l in range(self.ses.Lyr + 1):
                o[f"hs{l}"] = self.hidden(l).clone()
        return o


def assert_guards(named_arenas, what):
    for name, a in named_arenas:
        assert a.guards_intact(), f"{what}: a guard band of `{name}` ({a.nbytes} bytes) was written"


class Grads:
    """Gradient destinations.  present: hf_name -> bool (absent = True); a False entry is a NULL pointer.  adjacent_qkv: the
    q/k/v weight gradients of a block share one back-to-back buffer (what the Python host does) when all three are present.
    prior: hf_name -> CPU tensor the destination holds beforehand (accumulate); otherwise it holds `fill` (0xFF = NaN, so
    an element the backward did not write is not finite)."""

    def __init__(self, ses, present=None, adjacent_qkv=True, accumulate=0, prior=None, fill=0xFF):
        self.ses = ses
        present = present or {}
        Lb, cfg = ses.pkg.lib, ses.cfg
        self.shapes = ses.pkg.weights.param_shapes(cfg)
        self.t = {}          # hf_name -> fp32 tensor view of the destination
        self._arenas = []
        dev = ses.device

        def dest(names):
            n_el = [int(torch.Size(self.shapes[n]).numel()) for n in names]
            a = Arena(sum(n_el) * 4, fill, dev)
            self._arenas.append(("+".join(names), a))
            flat, off = a.f32(sum(n_el)), 0
            for n, k in zip(names, n_el):
                self.t[n] = flat[off:off + k].view(self.shapes[n])
                off += k
                if prior is not None and n in prior:
                    self.t[n].copy_(prior[n])

        want = lambda n: n in self.shapes and present.get(n, True)
        L = cfg.num_hidden_layers
        self._gl = (Lb.SglLayerPtrs * max(L, 1))()
        g = Lb.SglGrads()
        g.layers = C.cast(self._gl, C.POINTER(Lb.SglLayerPtrs))
        g.accumulate = int(accumulate)
        for l in range(L):
            qkv = [layer_name(l, f) for f in ("q_w", "k_w", "v_w")]
            if adjacent_qkv and all(want(n) for n in qkv):
                dest(qkv)
            for f in LAYER_NAMES:
                n = layer_name(l, f)
                if want(n) and n not in self.t:
                    dest([n])
                setattr(self._gl[l], f, self.t[n].data_ptr() if n in self.t else None)
        for f, n in list(GLOBAL_NAMES.items()) + list(HEAD_NAMES.items()):
            if want(n):
                dest([n])
            setattr(g, f, self.t[n].data_ptr() if n in self.t else None)
        self.struct = g

    def arenas(self):
        return self._arenas

    def cpu(self):
        return {n: t.detach().cpu().clone() for n, t in self.t.items()}

    def gpu(self):
        return {n: t.detach().clone() for n, t in self.t.items()}


# ------------------------------------------------------------------------------------------------------------------
# reference: the CPU oracle with the probe loss
# ------------------------------------------------------------------------------------------------------------------
def _cw(shape):
    n = int(torch.Size(shape).numel())
    return torch.cos(torch.arange(n, dtype=torch.float32).reshape(shape) * 0.37 + 0.11)


def upstream(B, N, D, L, taps):
    """oracle.probe_loss is linear in the outputs: its gradients w.r.t. pooled / last_hidden_state / hidden_states[i] are
    these constants (the d_pooled / d_last_hidden / d_taps the ABI takes)."""
    return {"pooled": _cw((B, D)), "last": 0.01 * _cw((B, N, D)), "taps": {int(i): 0.01 * _cw((B, N, D)) for i in taps}}


_REF_CACHE = {}


class Reference:
    """oracle.vision_forward in fp32 on the CPU with autograd, one graph per (config, seed, shape, ...) shared by every
    case that asks for it.  terms = (pooled, last, taps) present in the loss."""

    def __init__(self, pkg, oracle, cfg_name, seed, B, H, W, pixel_seed, taps, interp=True, terms=(1, 1, 1), use_head=1):
        cfg = make_config(pkg, cfg_name, use_head)
        sd = {k: v.clone().requires_grad_(True) for k, v in pkg.weights.seeded_state_dict(cfg, seed=seed).items()}
        x = pkg.weights.seeded_pixels(B, H, W, seed=pixel_seed)
        out = oracle.vision_forward(x, sd, cfg, True, interp)
        L, D = cfg.num_hidden_layers, cfg.hidden_size
        N = out["last_hidden_state"].shape[1]
        up = upstream(B, N, D, L, taps)
        loss = out["last_hidden_state"].sum() * 0.0
        if terms[0] and use_head:
            loss = loss + (out["pooler_output"] * up["pooled"]).sum()
        if terms[1]:
            loss = loss + (out["last_hidden_state"] * up["last"]).sum()
        if terms[2]:
            for i, u in up["taps"].items():
                loss = loss + (out["hidden_states"][i] * u).sum()
        if all(terms) and use_head:      # the scalar built above IS oracle.probe_loss
            pl = oracle.probe_loss(out, tuple(taps))
            assert abs(pl.item() - loss.item()) <= 1e-5 * max(1.0, abs(pl.item()))
        loss.backward()
        self.out = {"last": out["last_hidden_state"].detach().reshape(B * N, D)}
        if use_head:
            self.out["pooled"] = out["pooler_output"].detach()
        for l, h in enumerate(out["hidden_states"]):
            self.out[f"hs{l}"] = h.detach().reshape(B * N, D)
        self.grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in sd.items()}
        self.qscale = float(self.grads["encoder.layers.0.self_attn.q_proj.weight"].abs().max()) if L else 1.0
        self.N, self.up = N, up

    @classmethod
    def get(cls, *a, **kw):
        key = (a[2:], tuple(sorted(kw.items())))
        if key not in _REF_CACHE:
            _REF_CACHE[key] = cls(*a, **kw)
        return _REF_CACHE[key]

    def bar(self, name, mode):
        """tests/test_encoder_gpu.py, test_forward_backward_vs_hf_golden: fp32 1e-7 + 6e-5 * max|ref| per gradient tensor,
        bf16x3 six times that; k_proj.bias (an exact zero) judged against the q_proj.weight gradient's scale."""
        x3 = 6.0 if mode == "bf16x3" else 1.0
        assert mode in ("fp32", "bf16x3")
        if name.endswith("k_proj.bias"):
            return 6e-5 * x3 * self.qscale
        return 1e-7 + 6e-5 * x3 * float(self.grads[name].abs().max())

    def device_upstream(self, device, L, terms=(1, 1, 1)):
        """(d_last, d_pooled, d_taps list) on the device, None where the term is absent."""
        d_pooled = self.up["pooled"].to(device) if terms[0] and "pooled" in self.out else None
        d_last = self.up["last"].to(device).contiguous() if terms[1] else None
        d_taps = None
        if terms[2] and self.up["taps"]:
            d_taps = [self.up["taps"][l].to(device).contiguous() if l in self.up["taps"] else None for l in range(L + 1)]
        return d_last, d_pooled, d_taps
