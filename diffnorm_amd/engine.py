"""Thin Python handles over the C-ABI engine objects (DnEps / DnVae) of libdiffnorm_hip.so.

PyTorch is used only for device memory (packed weights, workspaces, I/O tensors) and the current
stream; all arithmetic runs in the HIP library.  There is no CPU path: constructing an engine
without a GPU or without the library raises.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, packing


def _dtype_code(dtype) -> int:
    if isinstance(dtype, str):
        names = {"bf16": _lib.DN_BF16, "f32": _lib.DN_F32, "fp32": _lib.DN_F32, "bf16x3": _lib.DN_BF16X3, "f16": _lib.DN_F16, "fp16": _lib.DN_F16}
        if dtype in names:
            return names[dtype]
    elif dtype is torch.bfloat16:
        return _lib.DN_BF16
    elif dtype is torch.float32:
        return _lib.DN_F32
    elif dtype is torch.float16:
        return _lib.DN_F16
    elif isinstance(dtype, int) and dtype in (_lib.DN_F32, _lib.DN_BF16, _lib.DN_BF16X3, _lib.DN_F16):
        return dtype
    raise ValueError(f"unsupported arithmetic dtype {dtype!r} (use 'bf16', 'f16', 'bf16x3' or 'f32')")


def _require_cuda(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.DiffNormHipError("diffnorm_amd engines need a HIP device (cuda:N); there is no CPU fallback")
    return device


def _i32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.int32).contiguous()


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def _loop_flags(use_graph: bool, split: bool = False, keep_table: bool = False) -> int:
    return (1 if use_graph else 0) | (2 if split else 0) | (4 if keep_table else 0)  # DN_LOOP_GRAPH | DN_LOOP_SPLIT2 | DN_LOOP_KEEP_TABLE


def capture_graph(device, step) -> torch.cuda.CUDAGraph:
    """`step()` captured into a hipGraph (torch.cuda.CUDAGraph over this library's launches on the capture stream); nothing runs.
    Capture happens on a side stream forked behind the current one (the null stream cannot capture) and joined back, so a replay on
    the current stream is ordered behind everything issued before this call.  The caller runs `step` eagerly once before (workspaces
    and kernel attributes settle outside capture) and keeps what it touches alive as long as the graph."""
    with torch.cuda.device(device):
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                step()
        cur.wait_stream(side)
    return g


class _Engine:
    def __init__(self, device, tensors: List[torch.Tensor]):
        self.device = _require_cuda(device)
        self.lib = _lib.load()
        self.tensors = [t.to(self.device).contiguous() for t in tensors]  # keeps packed weights alive
        self._table = (C.c_void_p * len(self.tensors))(*[t.data_ptr() for t in self.tensors])
        self._ws: Optional[torch.Tensor] = None
        self.handle = C.c_void_p()

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = _lib.alloc_workspace(nbytes, self.device)
        return self._ws

    _aligned = staticmethod(_lib.aligned)

    def _aligned_workspace(self, nbytes):
        return self._aligned(self._workspace(int(nbytes)))

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors)

    _kind = None     # "eps" / "vae": which of packing's inference lists `self.tensors` is
    _repack = None   # (layout key, device-resident DnRepackDesc array, number of descriptors, bytes read + written)

    def _repack_descs(self, train_engine):
        """The descriptors of dn_repack_weights for `train_engine`'s layout into this engine's packed tensors, built once per layout
        and kept on the device.  The plan is checked against the tensors it will write (count, shape, dtype) and the master
        buffer it will read, so a training engine of another configuration is refused here, on the host."""
        key = (tuple(train_engine.offsets), int(train_engine.n_params))
        if self._repack is not None and self._repack[0] == key:
            return self._repack
        plan = packing.repack_plan(train_engine.entries, train_engine.offsets, self.dtype, kind=self._kind)
        if len(plan.shapes) != len(self.tensors):
            raise ValueError(f"refresh_from: the training engine's layout gives {len(plan.shapes)} packed tensors, this engine has {len(self.tensors)}")
        for i, (s, t) in enumerate(zip(plan.shapes, self.tensors)):
            if s is not None and (tuple(t.shape) != tuple(s[0]) or t.dtype != s[1]):
                raise ValueError(f"refresh_from: packed tensor {i} is {tuple(t.shape)} {t.dtype}, the training engine's layout gives {s[0]} {s[1]}")
        descs = (_lib.RepackDesc * len(plan.items))()
        moved = 0
        for d, it in zip(descs, plan.items):
            n = it.mats * it.rows * it.K
            reads = n * max(1, it.count)
            assert 0 <= it.src and it.src + (reads if it.count else n) <= train_engine.n_params, it
            t = self.tensors[it.tensor]
            out_bytes = n * (4 if it.kind in (_lib.REPACK_COPY, _lib.REPACK_SUM) or not packing._is16(self.dtype) else 2)
            assert it.dst_byte + out_bytes <= t.numel() * t.element_size(), it
            # the alignment contract of include/diffnorm_hip.h: the kernel's 16-byte accesses assume it (only COPY falls back)
            dst = t.data_ptr() + it.dst_byte
            assert it.src % 4 == 0, it
            if it.kind in (_lib.REPACK_CONVERT, _lib.REPACK_KBLOCK):
                assert n % 32 == 0 and it.K % 32 == 0 and dst % 128 == 0, it
            elif it.kind == _lib.REPACK_SUM:
                assert it.K % 4 == 0 and it.stride % 4 == 0 and it.mats == it.rows == 1 and dst % 16 == 0, it
            d.src, d.dst, d.kind, d.mats, d.rows, d.K, d.count, d.stride = it.src, dst, it.kind, it.mats, it.rows, it.K, it.count, it.stride
            moved += reads * 4 + out_bytes
        dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.device)
        self._repack = (key, dev, len(plan.items), moved)
        return self._repack

    def _refresh_from(self, train_engine, source: str = "model"):
        """source: which flat fp32 buffer of the training engine is repacked -- "model" (master) or "ema" (its EMA, same layout: the
        descriptors are offsets into the buffer and serve both)."""
        if source not in ("model", "ema"):
            raise ValueError(f"refresh_from: source {source!r} (use 'model' or 'ema')")
        master = train_engine.master if source == "model" else getattr(train_engine, "ema", None)
        if master is None:
            raise ValueError("refresh_from: source 'ema' needs the training engine's EMA (enable_ema(), --store-ema)")
        if master.device != self.device or master.dtype != torch.float32 or not master.is_contiguous() or master.numel() != train_engine.n_params:
            raise ValueError("refresh_from: the training engine's master / EMA buffer must be a contiguous fp32 tensor of n_params elements on this engine's device")
        _, descs, n, _ = self._repack_descs(train_engine)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_repack_weights(master.data_ptr(), descs.data_ptr(), n, self.dtype, _lib.current_stream()), "dn_repack_weights")
        self._fold_from_flat(train_engine, master)

    # ---- the folded feed-forward weights (dn_ffn_fold), kept beside the packed table
    fold_W: Optional[torch.Tensor] = None
    fold_b: Optional[torch.Tensor] = None
    fold_Wkb: Optional[torch.Tensor] = None  # fold_W K-blocked (2-byte arithmetics): same sums, same bits, written by the same launch

    def _tf_dims(self):
        """(dim, depth) of the engine's transformer and the C entry that attaches its folded weights."""
        raise NotImplementedError

    def _attach_kblocked(self):
        """The C entry that attaches fold_Wkb."""
        raise NotImplementedError

    def _fold_call(self, srcs, strides, depth, layer0):
        dim, _, _ = self._tf_dims()
        inner = int(dim * 4 * 2 / 3)
        (_, _), b_shape = packing.ffn_fold_storage(dim, 1, self.dtype)
        w_off = layer0 * self.fold_W[0].numel() * self.fold_W.element_size()
        kb = None if self.fold_Wkb is None else self.fold_Wkb.data_ptr() + w_off  # (the two copies have the same bytes per layer)
        _lib.check(self.lib.dn_ffn_fold_kblocked(*srcs, *strides, depth, dim, inner, self.dtype, self.fold_W.data_ptr() + w_off,
                                                 self.fold_b.data_ptr() + layer0 * b_shape[1] * 4, kb, _lib.current_stream()), "dn_ffn_fold")

    def _fold_from_state_dict(self, tf_layers, sd):
        """Allocates the folded buffers, forms them layer by layer from the state dict's packed fp32 tensors and attaches them."""
        dim, depth, attach = self._tf_dims()
        (w_shape, w_dtype), b_shape = packing.ffn_fold_storage(dim, depth, self.dtype)
        with torch.cuda.device(self.device):
            self.fold_W = torch.empty(w_shape, dtype=w_dtype, device=self.device)
            self.fold_b = torch.empty(b_shape, dtype=torch.float32, device=self.device)
            if self.dtype in (_lib.DN_BF16, _lib.DN_F16):  # [depth][3][padk(inner)/32][padn(dim)][32]
                self.fold_Wkb = torch.empty((w_shape[0], 3, w_shape[3] // 32, w_shape[2], 32), dtype=w_dtype, device=self.device)
            for l, layer in enumerate(tf_layers):
                srcs = [t.to(self.device) for t in packing.ffn_fold_sources(layer, sd)]
                self._fold_call([t.data_ptr() for t in srcs], (0, 0, 0, 0), 1, l)
        _lib.check(attach(self.handle, self.fold_W.data_ptr(), self.fold_b.data_ptr()), "set_ffn_fold")
        if self.fold_Wkb is not None:
            _lib.check(self._attach_kblocked()(self.handle, self.fold_Wkb.data_ptr()), "set_ffn_fold_kblocked")

    def _fold_from_flat(self, train_engine, master):
        """The same entry on a training engine's flat fp32 buffer (master or EMA), after its repack: same sources, same bits."""
        if self.fold_W is None:
            return
        _, depth, _ = self._tf_dims()
        offs, strides = packing.ffn_fold_offsets(train_engine.entries, train_engine.offsets)
        with torch.cuda.device(self.device):
            self._fold_call([master.data_ptr() + 4 * o for o in offs], strides, depth, 0)

    def fold_bytes(self) -> int:
        return 0 if self.fold_W is None else sum(t.numel() * t.element_size() for t in (self.fold_W, self.fold_b, self.fold_Wkb) if t is not None)

    def refresh_bytes(self) -> int:
        """Bytes the last refresh_from's layout reads from the master plus writes to the packed tensors (0 before the first)."""
        return 0 if self._repack is None else self._repack[3]


class EpsEngine(_Engine):
    """eps-predictor `Model` (reference latent_module.py:709-876) on the GPU."""

    def __init__(self, state_dict, cfg, dtype="bf16", device="cuda:0", max_pos: int = 2048):
        self.cfg = cfg
        self.dtype = _dtype_code(dtype)
        super().__init__(device, packing.pack_eps(state_dict, cfg, self.dtype, max_pos))
        self.conditional = getattr(cfg, "dim_prompt", 0) > 0
        c = _lib.EpsConfig(cfg.dim, cfg.latent_dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.wavenet_layers,
                           cfg.wavenet_stacks, cfg.dim_cond_mult, self.dtype, max_pos, getattr(cfg, "dim_prompt", 0),
                           getattr(cfg, "num_latents_m", 0) if self.conditional else 0,
                           getattr(cfg, "resampler_depth", 0) if self.conditional else 0)
        _lib.check(self.lib.dn_eps_create(C.byref(c), self._table, len(self.tensors), C.byref(self.handle)),
                   "dn_eps_create")
        self._fold_from_state_dict(packing._eps_entries(cfg)[2], state_dict)

    def _tf_dims(self):
        return self.cfg.dim, self.cfg.depth, self.lib.dn_eps_set_ffn_fold

    def _attach_kblocked(self):
        return self.lib.dn_eps_set_ffn_fold_kblocked

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.dn_eps_destroy(self.handle)
            self.handle = None

    _kind = "eps"

    def refresh_from(self, train_engine, source: str = "model"):
        """Rewrites this engine's packed weights from `train_engine`'s (training.EpsTrainEngine) fp32 master buffer (source="ema": its
        EMA buffer) on the device
        (dn_repack_weights into the existing `self.tensors`): bit-identical to `EpsEngine(train_engine.state_dict(), ...)` in this
        engine's dtype, whatever the training dtype.  Stream-ordered on the current stream, no host synchronisation (the first call
        for a layout builds the descriptors and uploads them once).  The device addresses do not change.  What the engine derived
        from the weights, and what becomes of it:

        * the conditioning table of a chain (dn_ddim_loop / dn_ddpm_loop: the time-conditioning MLP and the stacked FiLM /
          adaptive-norm projections of every timestep, in the loop's workspace), which a `keep_table=True` continuation reuses:
          forgotten (dn_eps_weights_changed) -- the next call rebuilds it whatever `keep_table` says;
        * the captured hipGraph of the loop's step: kept.  It holds kernel launches over addresses (packed tensors, workspace,
          the conditioning table's rows), no values; every table it reads is rebuilt from the new weights before it is replayed;
        * the time table of a prompted chain (dn_eps_cond_time_table) lives for one `guided_ddim_chain` /
          `guided_ddim_schedule_loop` call only, and the prompt-conditioned engine has no training engine: refused here;
        * nothing else: the sinusoidal table and the placeholders do not depend on the parameters, workspaces hold activations."""
        if self.conditional:
            raise NotImplementedError("refresh_from covers the unconditional eps-predictor (the prompt-conditioned model has no training engine)")
        self._refresh_from(train_engine, source)
        _lib.check(self.lib.dn_eps_weights_changed(self.handle), "dn_eps_weights_changed")

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self.lib.dn_eps_workspace_bytes(self.handle, B, T))

    def forward(self, x: torch.Tensor, times: torch.Tensor, lengths: torch.Tensor, shared_t: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B,T,z] fp32, times [B] int, lengths [B] int -> eps_hat [B,T,z] fp32 (Model.forward :828-876)."""
        B, T, z = x.shape
        assert z == self.cfg.latent_dim
        x = _f32(x, self.device)
        t32, l32 = _i32(times, self.device), _i32(lengths, self.device)
        out = torch.empty_like(x) if out is None else out
        wp, wn = self._aligned_workspace(self.workspace_bytes(B, T))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_eps_forward(self.handle, x.data_ptr(), t32.data_ptr(), l32.data_ptr(), B, T,
                                               int(shared_t), out.data_ptr(), wp, wn, _lib.current_stream()),
                       "dn_eps_forward")
        return out

    def cond_time_table(self, t0: int, n_t: int) -> torch.Tensor:
        """The time half of the conditioning rows of timesteps t0 .. t0 + n_t - 1 (dn_eps_cond_time_table): fp32 [n_t, n_cond]."""
        n_cond = len(packing.eps_cond_modules(self.cfg)) * 2 * packing.padk(self.cfg.dim)
        table = torch.empty(n_t, n_cond, dtype=torch.float32, device=self.device)
        ws = _lib.alloc_workspace(self.lib.dn_eps_cond_time_table_workspace_bytes(self.handle, n_t), self.device)
        wp, wn = self._aligned(ws)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_eps_cond_time_table(self.handle, int(t0), int(n_t), table.data_ptr(), wp, wn, _lib.current_stream()),
                       "dn_eps_cond_time_table")
        return table

    def forward_cond(self, x: torch.Tensor, times: torch.Tensor, lengths: torch.Tensor, prompt: torch.Tensor, prompt_lengths: torch.Tensor,
                     drop: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, reuse_prompt: bool = False,
                     time_table: Optional[torch.Tensor] = None, table_t0: int = 0) -> torch.Tensor:
        """Conditional variant (reference Model.forward with condition_on_prompt, latent_module.py:828-876): prompt [B,Tp,dim_prompt],
        prompt_lengths [B]; drop [B] bool = the classifier-free-guidance drop mask (True: null condition).  Inside a chain:
        `reuse_prompt` skips the prompt-only work a previous call left in the workspace (same shapes, same prompt and drop mask),
        `time_table` (cond_time_table) supplies the time half of the conditioning rows."""
        B, T, z = x.shape
        Tp = prompt.shape[1]
        x, prompt = _f32(x, self.device), _f32(prompt, self.device)
        t32, l32, p32 = _i32(times, self.device), _i32(lengths, self.device), _i32(prompt_lengths, self.device)
        d32 = torch.zeros(B, dtype=torch.int32, device=self.device) if drop is None else _i32(drop, self.device)
        out = torch.empty_like(x) if out is None else out
        wp, wn = self._aligned_workspace(int(self.lib.dn_eps_cond_workspace_bytes(self.handle, B, T, Tp)))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_eps_forward_cond_ex(self.handle, x.data_ptr(), t32.data_ptr(), l32.data_ptr(), prompt.data_ptr(), p32.data_ptr(),
                                                       d32.data_ptr(), B, T, Tp, out.data_ptr(), wp, wn, int(bool(reuse_prompt)),
                                                       _lib.ptr(time_table), int(table_t0), 0 if time_table is None else time_table.shape[0],
                                                       _lib.current_stream()), "dn_eps_forward_cond")
        return out

    def _guided_inputs(self, lengths, prompt, prompt_lengths):
        """Static inputs of a guided pass over 2B rows = [conditioned ; null-conditioned] (the drop mask is per sample, :843-859)."""
        B = prompt.shape[0]
        two = lambda t: torch.cat([t, t]).contiguous()
        drop2 = torch.cat([torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32)]).to(self.device)
        return two(_i32(lengths, self.device)), two(_f32(prompt, self.device)), two(_i32(prompt_lengths, self.device)), drop2

    def forward_with_cond_scale(self, x, times, lengths, prompt, prompt_lengths, cond_scale: float = 1.0) -> torch.Tensor:
        """Classifier-free guidance (latent_module.py:813-826): null + (cond - null) * cond_scale.  The conditioned and the null pass
        are ONE launch sequence over 2B rows (the engine's drop mask is per sample); a scale of 1 needs the conditioned rows only."""
        B = x.shape[0]
        if cond_scale == 1.0:
            return self.forward_cond(x, times, lengths, prompt, prompt_lengths, torch.zeros(B, dtype=torch.bool))
        x = _f32(x, self.device)
        l2, p2, pl2, drop2 = self._guided_inputs(lengths, prompt, prompt_lengths)
        t2 = torch.cat([_i32(times, self.device)] * 2)
        both = self.forward_cond(torch.cat([x, x]).contiguous(), t2, l2, p2, pl2, drop2)
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_cfg_combine(both.data_ptr(), float(cond_scale), x.numel(), out.data_ptr(), _lib.current_stream()), "dn_cfg_combine")
        return out

    def guided_ddim_chain(self, x: torch.Tensor, lengths, prompt, prompt_lengths, start_step: int, coef: torch.Tensor, cond_scale: float = 1.0,
                          use_graph: bool = True, hoist: bool = True) -> int:
        """The prompted chain of the conditional variant, in place on x [B,T,z]: for t = start_step-1 .. 1 (t = 0 only when start_step
        == 1, like the reference's loop :1411-1445) the guided prediction (one 2B-row pass, or B rows at scale 1) and the DDIM eta = 0
        update.  One step -- timestep fill from a device counter, the pass, the guidance combination, the update, the decrement -- is
        captured into a hipGraph (torch.cuda.CUDAGraph over this library's launches on the capture stream) and replayed: the host only
        issues graph launches.  Returns the number of model evaluations."""
        from . import ops

        B, T, z = self._loop_x(x)
        guided = cond_scale != 1.0
        n = 2 * B if guided else B
        if guided:
            l2, p2, pl2, drop2 = self._guided_inputs(lengths, prompt, prompt_lengths)
        else:
            l2, p2, pl2 = _i32(lengths, self.device), _f32(prompt, self.device), _i32(prompt_lengths, self.device)
            drop2 = torch.zeros(B, dtype=torch.int32, device=self.device)
        tvec = torch.full((n,), start_step - 1, dtype=torch.int32, device=self.device)
        xin = torch.empty(n, T, z, dtype=torch.float32, device=self.device) if guided else x
        both = torch.empty(n, T, z, dtype=torch.float32, device=self.device)
        eps = torch.empty_like(x) if guided else both

        # prompt-only work (pooled-prompt half of the conditioning projection, resampler, every layer's prompt keys / values) once per
        # chain: the first step computes it into the workspace, every later step reuses it; the time half of the conditioning rows of
        # all the chain's steps comes from one table
        table = self.cond_time_table(0, start_step) if hoist else None
        first = [True]

        def one_step():
            if guided:
                xin[:B].copy_(x)
                xin[B:].copy_(x)
            self.forward_cond(xin, tvec, l2, p2, pl2, drop2, out=both, reuse_prompt=hoist and not first[0], time_table=table, table_t0=0)
            first[0] = False
            if guided:
                _lib.check(self.lib.dn_cfg_combine(both.data_ptr(), float(cond_scale), x.numel(), eps.data_ptr(), _lib.current_stream()), "dn_cfg_combine")
            ops.ddim_step(x, eps, coef, tvec[:B], T, out=x)
            tvec.sub_(1)

        n_eval = max(1, start_step - 1)
        with torch.cuda.device(self.device):
            one_step()  # eager first step: settles workspaces and kernel attributes outside capture
            done = 1
            if use_graph and n_eval > 2:
                g = capture_graph(self.device, one_step)  # (capture does not execute)
                for _ in range(n_eval - done):
                    g.replay()
                done = n_eval
            for _ in range(n_eval - done):
                one_step()
        return n_eval

    # ---- what the device sampling loops' wrappers share
    def _loop_x(self, x: torch.Tensor):
        assert x.is_contiguous() and x.dtype == torch.float32 and x.device == self.device
        return x.shape

    def _on_device(self, t: torch.Tensor, dtype, contiguous: bool = False) -> torch.Tensor:
        # (the loops' graph caches are keyed by device addresses: a copy where none is needed would turn a hit into a miss)
        if t.dtype == dtype and t.device == self.device and (t.is_contiguous() or not contiguous):
            return t
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _loop_schedule(self, steps: torch.Tensor, coef: torch.Tensor, cols: int) -> int:
        n = int(steps.shape[0])
        assert steps.dtype == torch.int32 and steps.is_contiguous() and steps.device == self.device and steps.dim() == 1
        assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.device == self.device and coef.shape == (n, cols)
        return n

    def _loop_noise(self, noise, shape, who: str = "", eta: Optional[float] = None):
        if noise is None:
            return None
        if eta is not None and not eta > 0:
            raise ValueError(f"{who}: injected noise needs eta > 0 (eta = 0 draws none)")
        nz = _f32(noise, self.device)
        assert nz.shape == shape, (nz.shape, shape)
        return nz

    def _loop_keys(self, keys, B: int, who: str, noise=None, seed: int = 0, eta: Optional[float] = None):
        """`keys` of a keyed chain: int64 [B] (the uint64 bit patterns of sharding.utterance_keys) -> the same on the device.  A
        tensor already there is passed as it is: the loops' graph caches are keyed by its address."""
        if keys is None:
            return None
        if noise is not None or int(seed) != 0:
            raise ValueError(f"{who}: keys draw the per-step noise: neither injected noise nor a non-zero seed can be given with them")
        if eta is not None and not eta > 0:
            raise ValueError(f"{who}: keys need eta > 0 (eta = 0 draws none)")
        if not (torch.is_tensor(keys) and keys.dtype == torch.int64 and tuple(keys.shape) == (B,)):
            raise ValueError(f"{who}: keys must be a torch.int64 tensor [{B}] (the uint64 bit patterns, one key per utterance)")
        return self._on_device(keys, torch.int64, contiguous=True)

    def ddim_loop(self, x: torch.Tensor, lengths: torch.Tensor, start_step: int, coef: torch.Tensor,
                  use_graph: bool = True, max_evals: int = 0, split: bool = True, keep_table: bool = False) -> int:
        """In-place DDIM eta=0 chain on x [B,T,z] fp32 (reference latent_module.py:1411-1445).
        coef: fp32 [timesteps,4] from `scheduler.ddim_coef_table`.  Returns the number of model evaluations.
        `max_evals` stops early; the caller continues with start_step - max_evals and may pass `keep_table=True` when
        nothing else used this engine in between (the conditioning table of the first call is then reused)."""
        B, T, z = self._loop_x(x)
        assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.device == self.device
        l32 = self._on_device(lengths, torch.int32)
        self._keep = (l32, coef)
        wp, wn = self._aligned_workspace(self.lib.dn_ddim_workspace_bytes(self.handle, B, T, start_step))
        with torch.cuda.device(self.device):
            return _lib.check(self.lib.dn_ddim_loop(self.handle, x.data_ptr(), l32.data_ptr(), B, T, start_step,
                                                    max_evals, coef.data_ptr(), coef.shape[0],
                                                    _loop_flags(use_graph, split, keep_table), wp, wn,
                                                    _lib.current_stream()), "dn_ddim_loop")

    def ddpm_loop(self, x: torch.Tensor, lengths: torch.Tensor, start_step: int, table: torch.Tensor, seed: int = 0,
                  noise: Optional[torch.Tensor] = None, clip_denoised: bool = False, use_graph: bool = True, max_evals: int = 0,
                  split: bool = True, keep_table: bool = False, keys: Optional[torch.Tensor] = None) -> int:
        """In-place ancestral (DDPM) chain on x [B,T,z] fp32: GaussianDiffusion.p_sample (reference diffusion/gaussian_diffusion.py:
        376-417) for t = start_step-1 .. 0, x given at index start_step-1 (x_T ~ N(0, I) with start_step = timesteps: BASELINE
        configs[2] read literally).  table: fp32 [timesteps, 12] from `scheduler.gaussian_table`.  The noise of a step is drawn
        in the update kernel (Philox keyed by `seed` and the step) or injected: noise [start_step, B, T, z], row k for
        t = start_step-1-k.  `keys` (int64 [B], excludes `noise` and a non-zero `seed`): the noise of row b at step t is
        `ops.randn_keyed`'s stream 2 + t of keys[b] (dn_ddpm_loop_keyed) -- it depends on the key, the timestep, the frame and the
        channel only, and both half batches draw it, so the keyed chain is split-invariant.  Returns the number of model evaluations."""
        B, T, z = self._loop_x(x)
        assert table.dtype == torch.float32 and table.is_contiguous() and table.device == self.device and table.shape[1] == 12
        l32 = self._on_device(lengths, torch.int32)
        nz = self._loop_noise(noise, (start_step, B, T, z))
        k64 = self._loop_keys(keys, B, "ddpm_loop", noise, seed)
        self._keep = (l32, table, nz, k64)
        wp, wn = self._aligned_workspace(self.lib.dn_ddim_workspace_bytes(self.handle, B, T, start_step))
        with torch.cuda.device(self.device):
            if k64 is not None:
                return _lib.check(self.lib.dn_ddpm_loop_keyed(self.handle, x.data_ptr(), l32.data_ptr(), B, T, start_step, max_evals,
                                                              table.data_ptr(), table.shape[0], int(clip_denoised), k64.data_ptr(),
                                                              _loop_flags(use_graph, split, keep_table), wp, wn,
                                                              _lib.current_stream()), "dn_ddpm_loop_keyed")
            return _lib.check(self.lib.dn_ddpm_loop(self.handle, x.data_ptr(), l32.data_ptr(), B, T, start_step, max_evals, table.data_ptr(),
                                                    table.shape[0], int(clip_denoised), int(seed) & (2 ** 64 - 1), _lib.ptr(nz),
                                                    _loop_flags(use_graph, split, keep_table), wp, wn,
                                                    _lib.current_stream()), "dn_ddpm_loop")

    def ddim_schedule_loop(self, x: torch.Tensor, lengths: torch.Tensor, steps: torch.Tensor, coef: torch.Tensor, eta: float = 0.0,
                           seed: int = 0, noise: Optional[torch.Tensor] = None, use_graph: bool = True, split: bool = True,
                           timesteps: Optional[int] = None, keys: Optional[torch.Tensor] = None) -> int:
        """In-place DDIM chain on x [B,T,z] fp32 over a timestep schedule (dn_ddim_sched_loop): `steps` int32 [n] strictly descending,
        `coef` fp32 [n, 5], both from `scheduler.ddim_schedule` (built with the same `eta`).  One evaluation per step; the
        conditioning table and the workspace have n rows.  eta > 0 adds sigma z after every update but one at timestep 0: z drawn
        in the update kernel (Philox keyed by `seed`, the step index and the element's index in the whole batch -- eager, graph and
        split chains agree bit for bit) or injected, noise [n, B, T, z], row i for update i.  `timesteps`: the length of the noise
        schedule the steps index (the entry refuses a list longer than that).  `keys` (int64 [B], needs eta > 0, excludes `noise`
        and a non-zero `seed`): z of row b at update i is `ops.randn_keyed`'s stream 2 + steps[i] of keys[b], drawn in the kernel
        (dn_ddim_sched_loop_keyed) -- it depends on the key, the timestep, the frame and the channel only, not on the batch.
        Returns the number of evaluations."""
        B, T, z = self._loop_x(x)
        n = self._loop_schedule(steps, coef, _lib.DDIM_SCHED_COLS)
        l32 = self._on_device(lengths, torch.int32)
        nz = self._loop_noise(noise, (n, B, T, z), "ddim_schedule_loop", eta)
        k64 = self._loop_keys(keys, B, "ddim_schedule_loop", noise, seed, eta)
        self._keep = (l32, steps, coef, nz, k64)
        wp, wn = self._aligned_workspace(self.lib.dn_ddim_sched_workspace_bytes(self.handle, B, T, n))
        with torch.cuda.device(self.device):
            if k64 is not None:
                return _lib.check(self.lib.dn_ddim_sched_loop_keyed(self.handle, x.data_ptr(), l32.data_ptr(), B, T, steps.data_ptr(),
                                                                    coef.data_ptr(), n, n if timesteps is None else int(timesteps),
                                                                    k64.data_ptr(), _loop_flags(use_graph, split), wp, wn,
                                                                    _lib.current_stream()), "dn_ddim_sched_loop_keyed")
            return _lib.check(self.lib.dn_ddim_sched_loop(self.handle, x.data_ptr(), l32.data_ptr(), B, T, steps.data_ptr(), coef.data_ptr(), n,
                                                          n if timesteps is None else int(timesteps), int(eta > 0), int(seed) & (2 ** 64 - 1), _lib.ptr(nz),
                                                          _loop_flags(use_graph, split), wp, wn, _lib.current_stream()),
                              "dn_ddim_sched_loop")

    def dpm_schedule_loop(self, x: torch.Tensor, lengths: torch.Tensor, steps: torch.Tensor, rows: torch.Tensor, use_graph: bool = True,
                          split: bool = True, timesteps: Optional[int] = None) -> int:
        """In-place DPM-Solver++(2M) chain on x [B,T,z] fp32 over a timestep schedule (dn_dpm_loop): `steps` int32 [n] strictly
        descending and `rows` fp32 [n, 6], both from `scheduler.dpm_schedule`.  `ddim_schedule_loop`'s chain -- one evaluation per
        step, conditioning table of n rows, hipGraph replay, two half-batch streams -- with the second-order multistep update; the
        workspace holds one more latent-sized buffer, the previous step's data prediction.  Deterministic: no eta, no noise.  `steps`
        may also be a list or a host tensor: it is then validated by dn_ddim_sched_check against `timesteps` and uploaded.
        Returns the number of evaluations."""
        B, T, z = self._loop_x(x)
        nt = None if timesteps is None else int(timesteps)
        if not (isinstance(steps, torch.Tensor) and steps.device == self.device):
            host = torch.as_tensor(steps, dtype=torch.int32).contiguous().view(-1)
            if self.lib.dn_ddim_sched_check(host.data_ptr() if host.numel() else None, int(host.numel()),
                                            int(host.numel()) if nt is None else nt) != 0:
                raise ValueError("dpm_schedule_loop: " + (self.lib.dn_last_error() or b"").decode())
            steps = host.to(self.device)
        n = self._loop_schedule(steps, rows, _lib.DPM_COLS)
        l32 = self._on_device(lengths, torch.int32)
        self._keep = (l32, steps, rows)
        wp, wn = self._aligned_workspace(self.lib.dn_dpm_workspace_bytes(self.handle, B, T, n))
        with torch.cuda.device(self.device):
            return _lib.check(self.lib.dn_dpm_loop(self.handle, x.data_ptr(), l32.data_ptr(), B, T, steps.data_ptr(), rows.data_ptr(), n,
                                                   n if nt is None else nt, _loop_flags(use_graph, split), wp, wn,
                                                   _lib.current_stream()), "dn_dpm_loop")

    def gaussian_loop(self, x: torch.Tensor, lengths: torch.Tensor, steps: torch.Tensor, table: torch.Tensor, sampler: str = "p_sample",
                      clip_denoised: bool = True, eta: float = 0.0, seed: int = 0, noise: Optional[torch.Tensor] = None,
                      keys: Optional[torch.Tensor] = None, graph: bool = True, split: bool = True, timesteps: Optional[int] = None) -> int:
        """In-place chain of the generic Gaussian scheduler on x [B,T,z] fp32 (dn_gaussian_loop): GaussianDiffusion.p_sample_loop
        (`sampler="p_sample"`) or ddim_sample_loop (`"ddim"`, with `eta`) of a respaced or plain diffusion.  `steps` int32 [n]: the
        ORIGINAL timesteps, strictly descending; `table` fp32 [n, 12]: the respaced diffusion's `gaussian_table` rows in the same
        order, so the last row is respaced index 0 and adds no noise.  The noise of update i is drawn in the kernel (Philox keyed by
        `seed`, i and the element's index in the whole batch -- eager, graph and split chains agree bit for bit), injected (`noise`
        [n, B, T, z], row i), or keyed (`keys` int64 [B]; excludes `noise` and a non-zero `seed`): `ops.randn_keyed`'s stream
        2 + steps[i] of keys[b], which depends on the key, the original timestep, the frame and the channel only.  `steps` may also
        be a list or a host tensor: it is then validated by dn_ddim_sched_check against `timesteps` and uploaded.  `timesteps`: the
        length of the original noise schedule.  Returns the number of evaluations."""
        if sampler not in ("p_sample", "ddim"):
            raise ValueError(f"gaussian_loop: unknown sampler {sampler!r} ('p_sample' or 'ddim')")
        B, T, z = self._loop_x(x)
        nt = None if timesteps is None else int(timesteps)
        if not (isinstance(steps, torch.Tensor) and steps.device == self.device):
            host = torch.as_tensor(steps, dtype=torch.int32).contiguous().view(-1)
            limit = nt if nt is not None else (int(host.max()) + 1 if host.numel() else 0)  # (unset: only the order is checked)
            if self.lib.dn_ddim_sched_check(host.data_ptr() if host.numel() else None, int(host.numel()), limit) != 0:
                raise ValueError("gaussian_loop: " + (self.lib.dn_last_error() or b"").decode())
            steps = host.to(self.device)
        n = self._loop_schedule(steps, table, _lib.GD_COLS)
        l32 = self._on_device(lengths, torch.int32)
        nz = self._loop_noise(noise, (n, B, T, z))
        k64 = self._loop_keys(keys, B, "gaussian_loop", noise, seed)
        self._keep = (l32, steps, table, nz, k64)
        wp, wn = self._aligned_workspace(self.lib.dn_gaussian_workspace_bytes(self.handle, B, T, n))
        head = (self.handle, x.data_ptr(), l32.data_ptr(), B, T, steps.data_ptr(), table.data_ptr(), n, n if nt is None else nt,
                int(sampler == "ddim"), int(bool(clip_denoised)), float(eta))
        with torch.cuda.device(self.device):
            if k64 is not None:
                return _lib.check(self.lib.dn_gaussian_loop_keyed(*head, k64.data_ptr(), _loop_flags(graph, split), wp, wn,
                                                                  _lib.current_stream()), "dn_gaussian_loop_keyed")
            return _lib.check(self.lib.dn_gaussian_loop(*head, int(seed) & (2 ** 64 - 1), _lib.ptr(nz), _loop_flags(graph, split), wp, wn,
                                                        _lib.current_stream()), "dn_gaussian_loop")

    def cond_time_table_steps(self, steps) -> torch.Tensor:
        """The time half of the conditioning rows of the timesteps `steps` (any list or int tensor; dn_eps_cond_time_table_steps):
        fp32 [n, n_cond], row i for steps[i]."""
        st = _i32(torch.as_tensor(steps), self.device)
        assert st.dim() == 1 and st.numel() > 0
        n = int(st.numel())
        n_cond = len(packing.eps_cond_modules(self.cfg)) * 2 * packing.padk(self.cfg.dim)
        table = torch.empty(n, n_cond, dtype=torch.float32, device=self.device)
        ws = _lib.alloc_workspace(self.lib.dn_eps_cond_time_table_workspace_bytes(self.handle, n), self.device)
        wp, wn = self._aligned(ws)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_eps_cond_time_table_steps(self.handle, st.data_ptr(), n, table.data_ptr(), wp, wn, _lib.current_stream()),
                       "dn_eps_cond_time_table_steps")
        return table

    def guided_ddim_schedule_loop(self, x: torch.Tensor, lengths, prompt, prompt_lengths, steps: torch.Tensor, coef: torch.Tensor,
                                  cond_scale: float = 1.0, eta: float = 0.0, seed: int = 0, noise: Optional[torch.Tensor] = None,
                                  use_graph: bool = True, timesteps: Optional[int] = None, keys: Optional[torch.Tensor] = None) -> int:
        """In-place prompted, guided DDIM chain on x [B,T,z] fp32 over a timestep schedule (dn_guided_ddim_loop): `ddim_schedule_loop`'s
        chain -- `steps` int32 [n] strictly descending and `coef` fp32 [n, 5] from `scheduler.ddim_schedule` (built with the same
        `eta`), `seed`, injected `noise` [n, B, T, z], `timesteps` with its meaning -- with the guided prediction of
        `forward_with_cond_scale` (one pass over 2B rows, or B rows at scale 1).  The whole loop runs behind the C entry: time table
        of n rows, prompt-only work in the first step, one fused combination + update kernel per step, hipGraph replay.  On the
        every-timestep schedule at eta = 0 it is `guided_ddim_chain` bit for bit.  `keys` as `ddim_schedule_loop` takes them
        (dn_guided_ddim_loop_keyed).  Returns the number of evaluations."""
        B, T, z = self._loop_x(x)
        n = self._loop_schedule(steps, coef, _lib.DDIM_SCHED_COLS)
        l32 = self._on_device(lengths, torch.int32)
        pl32 = self._on_device(prompt_lengths, torch.int32)
        p32 = self._on_device(prompt, torch.float32, contiguous=True)
        assert p32.dim() == 3 and p32.shape[0] == B and p32.shape[2] == self.cfg.dim_prompt and l32.shape == (B,) and pl32.shape == (B,)
        Tp = int(p32.shape[1])
        nz = self._loop_noise(noise, (n, B, T, z), "guided_ddim_schedule_loop", eta)
        k64 = self._loop_keys(keys, B, "guided_ddim_schedule_loop", noise, seed, eta)
        self._keep = (l32, pl32, p32, steps, coef, nz, k64)
        wp, wn = self._aligned_workspace(self.lib.dn_guided_ddim_workspace_bytes(self.handle, B, T, Tp, n, int(float(cond_scale) != 1.0)))
        with torch.cuda.device(self.device):
            if k64 is not None:
                return _lib.check(self.lib.dn_guided_ddim_loop_keyed(self.handle, x.data_ptr(), l32.data_ptr(), p32.data_ptr(), pl32.data_ptr(), B,
                                                                     T, Tp, float(cond_scale), steps.data_ptr(), coef.data_ptr(), n,
                                                                     n if timesteps is None else int(timesteps), k64.data_ptr(),
                                                                     _loop_flags(use_graph), wp, wn, _lib.current_stream()),
                                  "dn_guided_ddim_loop_keyed")
            return _lib.check(self.lib.dn_guided_ddim_loop(self.handle, x.data_ptr(), l32.data_ptr(), p32.data_ptr(), pl32.data_ptr(), B, T, Tp,
                                                           float(cond_scale), steps.data_ptr(), coef.data_ptr(), n,
                                                           n if timesteps is None else int(timesteps), int(eta > 0), int(seed) & (2 ** 64 - 1),
                                                           _lib.ptr(nz), _loop_flags(use_graph), wp, wn, _lib.current_stream()),
                              "dn_guided_ddim_loop")

    def guided_dpm_schedule_loop(self, x: torch.Tensor, lengths, prompt, prompt_lengths, steps: torch.Tensor, rows: torch.Tensor,
                                 cond_scale: float = 1.0, use_graph: bool = True, timesteps: Optional[int] = None) -> int:
        """In-place prompted, guided DPM-Solver++(2M) chain on x [B,T,z] fp32 over a timestep schedule (dn_guided_dpm_loop):
        `guided_ddim_schedule_loop`'s chain -- the guided prediction of `forward_with_cond_scale` over 2B rows (B at scale 1), time
        table of n rows, prompt-only work in the first step, one fused combination + update kernel per step, hipGraph replay -- with
        `dpm_schedule_loop`'s update: `steps` int32 [n] strictly descending and `rows` fp32 [n, 6], both from
        `scheduler.dpm_schedule`; the workspace holds one more latent-sized buffer, the previous step's data prediction.
        Deterministic: no eta, no noise.  `steps` may also be a list or a host tensor: it is then validated by dn_ddim_sched_check
        against `timesteps` and uploaded.  Returns the number of evaluations."""
        B, T, z = self._loop_x(x)
        nt = None if timesteps is None else int(timesteps)
        if not (isinstance(steps, torch.Tensor) and steps.device == self.device):
            host = torch.as_tensor(steps, dtype=torch.int32).contiguous().view(-1)
            if self.lib.dn_ddim_sched_check(host.data_ptr() if host.numel() else None, int(host.numel()),
                                            int(host.numel()) if nt is None else nt) != 0:
                raise ValueError("guided_dpm_schedule_loop: " + (self.lib.dn_last_error() or b"").decode())
            steps = host.to(self.device)
        n = self._loop_schedule(steps, rows, _lib.DPM_COLS)
        l32 = self._on_device(lengths, torch.int32)
        pl32 = self._on_device(prompt_lengths, torch.int32)
        p32 = self._on_device(prompt, torch.float32, contiguous=True)
        assert p32.dim() == 3 and p32.shape[0] == B and p32.shape[2] == self.cfg.dim_prompt and l32.shape == (B,) and pl32.shape == (B,)
        Tp = int(p32.shape[1])
        self._keep = (l32, pl32, p32, steps, rows)
        wp, wn = self._aligned_workspace(self.lib.dn_guided_dpm_workspace_bytes(self.handle, B, T, Tp, n, int(float(cond_scale) != 1.0)))
        with torch.cuda.device(self.device):
            return _lib.check(self.lib.dn_guided_dpm_loop(self.handle, x.data_ptr(), l32.data_ptr(), p32.data_ptr(), pl32.data_ptr(), B, T, Tp,
                                                          float(cond_scale), steps.data_ptr(), rows.data_ptr(), n, n if nt is None else nt,
                                                          _loop_flags(use_graph), wp, wn, _lib.current_stream()), "dn_guided_dpm_loop")


class VaeEngine(_Engine):
    """SpeechVAEEncoderDecoder (reference latent_module.py:1035-1142) on the GPU."""

    def __init__(self, state_dict, dim: int = 768, latent_dim: int = 128, dtype="bf16", device="cuda:0",
                 depth: int = 6, heads: int = 8, dim_head: int = 96, stacks: int = 2, layers: int = 3,
                 vocab: int = 1004):
        self.dim, self.vocab = dim, vocab
        self.mults = packing.vae_mults(latent_dim)
        z = dim
        for m in self.mults:
            z //= m
        self.z = z // 2
        self.dtype = _dtype_code(dtype)
        super().__init__(device, packing.pack_vae(state_dict, dim, self.mults, depth, heads, dim_head, stacks, layers,
                                                  vocab, self.dtype))
        mults = (C.c_int32 * 4)(*(self.mults + [0] * (4 - len(self.mults))))
        c = _lib.VaeConfig(dim, self.z, depth, heads, dim_head, stacks, layers, vocab, len(self.mults), mults, self.dtype)
        _lib.check(self.lib.dn_vae_create(C.byref(c), self._table, len(self.tensors), C.byref(self.handle)),
                   "dn_vae_create")
        self._tf = (dim, depth)
        self._fold_from_state_dict(packing._vae_entries(dim, self.mults, depth, heads, dim_head, stacks, layers, vocab)[1], state_dict)

    def _tf_dims(self):
        return self._tf[0], self._tf[1], self.lib.dn_vae_set_ffn_fold

    def _attach_kblocked(self):
        return self.lib.dn_vae_set_ffn_fold_kblocked

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.dn_vae_destroy(self.handle)
            self.handle = None

    _kind = "vae"

    def refresh_from(self, train_engine, source: str = "model"):
        """Rewrites this engine's packed weights from `train_engine`'s (training.VaeTrainEngine: f32, bf16 or bf16x3) fp32 master
        buffer (source="ema": its EMA buffer) on the device: bit-identical to `VaeEngine(train_engine.state_dict(), ...)` in this engine's dtype.  Stream-ordered,
        no host synchronisation, same device addresses (see EpsEngine.refresh_from).  The VAE engine derives nothing from its
        weights (DnVae holds the table's pointers only; no graph, no table), so there is nothing to invalidate."""
        self._refresh_from(train_engine, source)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self.lib.dn_vae_workspace_bytes(self.handle, B, T))

    def encode_params(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [B,T,dim] fp32 -> posterior parameters [B,T,2z] fp32 ([mean ; logvar])."""
        B, T, _ = feat.shape
        feat = _f32(feat, self.device)
        out = torch.empty(B, T, 2 * self.z, dtype=torch.float32, device=self.device)
        wp, wn = self._aligned_workspace(self.workspace_bytes(B, T))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_vae_encode_params(self.handle, feat.data_ptr(), B, T, out.data_ptr(), wp, wn,
                                                     _lib.current_stream()), "dn_vae_encode_params")
        return out

    def sample_posterior(self, params: torch.Tensor, noise: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                         want_kl: bool = False):
        """DiagonalGaussianDistribution.sample / kl_3d (reference distributions.py:24-41, 62-74)."""
        B, T, _ = params.shape
        noise = _f32(noise, self.device)
        z = torch.empty(B, T, self.z, dtype=torch.float32, device=self.device)
        kl_rows = torch.empty(B, T, dtype=torch.float32, device=self.device) if want_kl else None
        l32 = _i32(lengths, self.device) if lengths is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_posterior_sample(params.data_ptr(), 2 * self.z, noise.data_ptr(), self.z, z.data_ptr(),
                                                    None, _lib.DN_F32, self.z, B * T, self.z, T, _lib.ptr(l32),
                                                    _lib.ptr(kl_rows), _lib.current_stream()), "dn_posterior_sample")
        if want_kl:
            return z, kl_rows.sum(dim=1) / (T * self.z)  # mean over (z,T) with pads counted, per sample
        return z

    def encode(self, feat: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """encode_feature (reference latent_module.py:1099-1107) with caller-supplied posterior noise."""
        return self.sample_posterior(self.encode_params(feat), noise)

    def decode(self, latent: torch.Tensor, lengths: torch.Tensor, want_recon=True, want_logits=True, want_units=True):
        """decode_feature (:1109-1116) -> (recon [B,T,dim], logits [B,T,vocab], units [B,T] = argmax-4)."""
        B, T, _ = latent.shape
        latent = _f32(latent, self.device)
        l32 = _i32(lengths, self.device)
        recon = torch.empty(B, T, self.dim, dtype=torch.float32, device=self.device) if want_recon else None
        logits = torch.empty(B, T, self.vocab, dtype=torch.float32, device=self.device) if want_logits else None
        units = torch.empty(B, T, dtype=torch.int32, device=self.device) if want_units else None
        wp, wn = self._aligned_workspace(self.workspace_bytes(B, T))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_vae_decode(self.handle, latent.data_ptr(), l32.data_ptr(), B, T, _lib.ptr(recon),
                                              _lib.ptr(logits), _lib.ptr(units), wp, wn, _lib.current_stream()),
                       "dn_vae_decode")
        return recon, logits, units
