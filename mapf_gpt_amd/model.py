"""Host mirror of the reference policy class (mapf_gpt/model.py) over the HIP forward.

`GPTConfig` / `GPT` keep the reference's names and call shapes for the inference surface:
    GPT(config); load_state_dict(sd, strict=False); to(device); eval();
    forward(idx) -> (logits [B,1,67], None)        (model.py:167-189, last position only)
    forward(idx, targets) -> (logits [B,T,67], loss)  (model.py:180-184: every position, cross-entropy with ignore_index=-1)
    act(idx, do_sample=True, generator=None) -> LongTensor [B]   (model.py:244-260)
plus the device-resident fast path `act_tokens(tokens_u8, ...)` used by the batched runner.
`score_tokens` and mapf_gpt_amd/scoring.py score a checkpoint on expert data (train.py estimate_loss).
Training (train.py:324-331) runs on the device in exact fp32 or in train.py's bf16 autocast regime (forward_backward(...,
precision="bf16")): train(), forward_backward(idx, targets), zero_grad(),
clip_grad_norm_(), grads(), state_dict() and configure_optimizers() -> AdamW (model.py:202-226); data-parallel runs (train.py:237-239)
synchronise through grads_size(), export_grads() and reduce_grads(): a gather and a rank-ordered sum, no DDP wrapper.  estimate_mfu and
crop_block_size are out of scope.  Every compute call goes through the C ABI; there is no PyTorch forward here.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, weights


@dataclass
class GPTConfig:          # = model.py:107-115 (same field names and defaults)
    block_size: int = 161
    vocab_size: int = 67
    n_layer: int = 8
    n_head: int = 8
    n_embd: int = 256
    dropout: float = 0.0
    bias: bool = False


class GPT:
    ENVELOPE_POLICIES = {"fallback": 0, "refuse": 1, "ignore": 2}      # include/mapf_gpt_amd.h: MGPT_ENVELOPE_*

    def __init__(self, config, max_rows=2048, precision="f32", device="cuda", envelope="fallback"):
        if config.vocab_size != 67:
            raise ValueError("vocab_size must be 67 (observation_generator.cpp:321-344)")
        # bias=True (model.py:115; no released config uses it): the checkpoint's *.bias tensors are loaded like any other and carried by the
        # exact-fp32 kernels -- precision="f16x3" then follows the envelope policy (fallback: fp32), "bf16" raises (include/mapf_gpt_amd.h)
        if not (0.0 <= config.dropout < 1.0):
            raise ValueError("dropout must be in [0, 1)")
        # dropout: the identity on every inference and scoring path -- the reference serves every model in eval mode (inference.py:85
        # net.eval(): nn.Dropout and scaled_dot_product_attention's dropout_p are the identity there, model.py:33-34,59,82,129); only
        # forward_backward in training mode applies it
        self.config = config
        self.max_rows = int(max_rows)
        self.precision = precision
        if envelope not in self.ENVELOPE_POLICIES:
            raise ValueError(f"envelope must be one of {sorted(self.ENVELOPE_POLICIES)}")
        # what happens to precision="f16x3" requests when the loaded checkpoint lies outside the range on which that mode's 1e-5
        # logit bar was established: "fallback" = serve them with the exact-fp32 kernels (one line on stderr), "refuse" = raise,
        # "ignore" = run the split path regardless (parity experiments).  See include/mapf_gpt_amd.h, mgpt_gpt_envelope.
        self.envelope_policy = envelope
        self.device = torch.device(device)
        self._h = None
        self._loaded = False
        self.training = False
        self._act_calls = 0          # advances the library RNG between generator-less act() calls

    # ---- lifecycle -------------------------------------------------------------------------
    def _ensure(self):
        if self._h is None:
            _lib.require_gpu()
            h = ctypes.c_void_p()
            c = self.config
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mgpt_gpt_create(ctypes.byref(h), c.n_layer, c.n_head, c.n_embd, c.block_size, self.max_rows))
            self._h = h
            _lib.check(_lib.lib().mgpt_gpt_set_envelope_policy(h, self.ENVELOPE_POLICIES[self.envelope_policy]))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().mgpt_gpt_destroy(h)
            except Exception:      # interpreter shutdown: module globals may already be gone
                pass
            self._h = None

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mapf_gpt_amd.GPT runs on a HIP device only (no CPU forward in this package)")
        if self._h is not None and device != self.device and device.index is not None:
            raise RuntimeError("move the model before loading weights")
        self.device = device
        return self

    def eval(self):
        self.training = False
        return self

    def load_state_dict(self, state_dict, strict=False):
        """Accepts the reference checkpoint's state_dict (tensors or arrays, `_orig_mod.` prefixes allowed,
        inference.py:33-44).  strict=False (the reference's choice, inference.py:83) skips unknown keys."""
        self._ensure()
        sd = weights.strip_prefix(state_dict)
        unknown = []
        for k, v in sd.items():
            if k.endswith(".bias") and not self.config.bias:      # a bias=False module has no such parameter: an unexpected key (model.py:14-17,29)
                unknown.append(k)
                continue
            a = v.detach().to(torch.float32).cpu().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)
            a = np.ascontiguousarray(a)
            rc = _lib.lib().mgpt_gpt_set_param(self._h, k.encode(), ctypes.c_void_p(a.ctypes.data), a.size, 0)
            if rc == _lib.ERR_ARG and b"unknown parameter" in _lib.lib().mgpt_last_error():
                unknown.append(k)
                continue
            _lib.check(rc)
        if strict and unknown:
            raise KeyError(f"unexpected keys: {unknown}")
        _lib.check(_lib.lib().mgpt_gpt_finalize(self._h))
        self._loaded = True
        return unknown

    def envelope(self):
        """Precision envelope of the loaded checkpoint: {max_abs_w, max_rms_w (over the block matrices), probe_err (max |f16x3 - f32|
        over the probe rows' logits, None before the first f16x3 forward), state: "undecided" | "inside" | "outside",
        effective_precision: what a precision="f16x3" request runs}."""
        assert self._loaded, "load_state_dict first"
        out, st = (ctypes.c_float * 3)(), ctypes.c_int(0)
        _lib.check(_lib.lib().mgpt_gpt_envelope(self._h, out, ctypes.byref(st)))
        state = ("undecided", "inside", "outside")[st.value]
        eff = "f32" if (state == "outside" and self.envelope_policy == "fallback") else "f16x3"
        pr = (ctypes.c_float * 4)()
        _lib.check(_lib.lib().mgpt_gpt_envelope_probe(self._h, pr))
        return {"max_abs_w": float(out[0]), "max_rms_w": float(out[1]), "probe_err": (None if out[2] < 0 else float(out[2])),
                "probe_err_small_calls": (None if pr[0] < 0 else float(pr[0])), "probe_err_large_calls": (None if pr[1] < 0 else float(pr[1])),
                "probe_tol": (None if out[2] < 0 else float(pr[2])), "probe_max_logit": (None if out[2] < 0 else float(pr[3])),
                "state": state, "policy": self.envelope_policy, "effective_precision": eff}

    # ---- compute ---------------------------------------------------------------------------
    def _prec(self, precision):
        return _lib.PRECISIONS[precision or self.precision]

    def _tokens_u8(self, idx):
        # model.py:168-170: any t <= block_size.  256-token rows (what the tokenizer emits, inference.py:145) take the model's kernels of its
        # precision; shorter rows are served by the exact-fp32 kernels (mgpt_gpt_forward_t)
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError(f"idx must be [B, T] token rows, got {tuple(idx.shape)}")
        if idx.shape[1] > self.config.block_size:
            raise ValueError(f"Cannot forward sequence of length {idx.shape[1]}, block size is only {self.config.block_size}")
        return idx.to(device=self.device, dtype=torch.uint8).contiguous()

    def logits_tokens_t(self, tokens_u8, out=None):
        """tokens uint8 [rows, T <= block_size] on the device -> float32 [rows, 67]: the logits of position T - 1 (model.py:186), exact-fp32 kernels."""
        assert self._loaded, "load_state_dict first"
        rows, T = tokens_u8.shape
        if out is None:
            out = torch.empty((rows, 67), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_forward_t(self._h, _lib.ptr(tokens_u8), rows, T, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def _logits(self, tokens_u8):
        return self.logits_tokens(tokens_u8) if tokens_u8.shape[1] == 256 else self.logits_tokens_t(tokens_u8)

    def logits_tokens(self, tokens_u8, precision=None, out=None):
        """tokens uint8 [rows, 256] on the device -> float32 [rows, 67] (last-position logits)."""
        assert self._loaded, "load_state_dict first"
        rows = tokens_u8.shape[0]
        if out is None:
            out = torch.empty((rows, 67), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_forward(self._h, _lib.ptr(tokens_u8), rows, _lib.ptr(out), self._prec(precision),
                                                   _lib.stream_ptr()))
        return out

    def act_tokens(self, tokens_u8, do_sample=True, seed=0, step=0, precision=None, out=None, logits_out=None, row0=0):
        """Fused forward + 5-way masked softmax + sampling on the device (library RNG keyed by
        (seed, step, row0 + row); row0 = global id of the first row when the caller holds a shard) -> int32 [rows]."""
        assert self._loaded, "load_state_dict first"
        rows = tokens_u8.shape[0]
        if out is None:
            out = torch.empty((rows,), dtype=torch.int32, device=self.device)
        lp = _lib.ptr(logits_out) if logits_out is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_act(self._h, _lib.ptr(tokens_u8), rows, _lib.ptr(out), lp, 1 if do_sample else 0,
                                               int(seed) & (2 ** 64 - 1), int(step), int(row0), self._prec(precision), _lib.stream_ptr()))
        return out

    def forward(self, idx, targets=None):
        tokens = self._tokens_u8(idx)
        if targets is None:
            logits = self._logits(tokens)
            return logits[:, None, :], None
        return self._forward_seq(tokens, targets)

    def _forward_seq(self, tokens, targets):
        # model.py:180-184: lm_head on every position, F.cross_entropy(logits.view(-1, 67), targets.view(-1), ignore_index=-1).  Evaluation only:
        # no graph, no backward (train.py:244-257 estimate_loss runs it under no_grad)
        assert self._loaded, "load_state_dict first"
        B, T = tokens.shape
        targets = torch.as_tensor(targets)
        if targets.dtype.is_floating_point or targets.dtype == torch.bool or targets.numel() != B * T:
            raise ValueError(f"targets must be an integer tensor of {B * T} elements (idx is {B} x {T}), got {targets.dtype} {tuple(targets.shape)}")
        if targets.numel() and (int(targets.min()) < -1 or int(targets.max()) >= 67):
            raise ValueError("targets must lie in [-1, 67): -1 is ignored (ignore_index=-1), 0 .. 66 are vocabulary ids")
        tg = targets.reshape(B, T).to(device=self.device, dtype=torch.int32).contiguous()
        logits = torch.empty((B, T, 67), dtype=torch.float32, device=self.device)
        nll = torch.empty((B,), dtype=torch.float32, device=self.device)
        cnt = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_forward_seq(self._h, _lib.ptr(tokens), B, T, _lib.ptr(logits), _lib.ptr(tg), _lib.ptr(nll), _lib.ptr(cnt),
                                                       self._prec(None), _lib.stream_ptr()))
        # mean over the targeted positions; 0 / 0 = NaN when every target is -1, as F.cross_entropy gives
        loss = (nll.double().sum() / cnt.sum().double()).float()
        return logits, loss

    def score_tokens(self, tokens_u8, actions, precision=None, logits_out=None):
        """Scoring of 256-token rows against one expert action each (dataset gt_actions): the forward of act_tokens (same kernels, same
        logits) -> (nll float32 [N] = -log softmax(logits)[action] over all 67 logits, hit bool [N] = greedy action == action), on the device.
        A hit agrees with act_tokens(do_sample=False) == action bit for bit."""
        assert self._loaded, "load_state_dict first"
        rows = tokens_u8.shape[0]
        actions = torch.as_tensor(actions)
        if actions.dtype.is_floating_point or actions.numel() != rows:
            raise ValueError(f"actions must be {rows} integers, got {actions.dtype} {tuple(actions.shape)}")
        if rows and (int(actions.min()) < 0 or int(actions.max()) >= 67):
            raise ValueError("actions must lie in [0, 67)")
        tg = actions.reshape(rows).to(device=self.device, dtype=torch.int32).contiguous()
        nll = torch.empty((rows,), dtype=torch.float32, device=self.device)
        hit = torch.empty((rows,), dtype=torch.int32, device=self.device)
        lp = _lib.ptr(logits_out) if logits_out is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_score_last(self._h, _lib.ptr(tokens_u8), rows, _lib.ptr(tg), _lib.ptr(nll), _lib.ptr(hit), lp,
                                                      self._prec(precision), _lib.stream_ptr()))
        return nll, hit.bool()

    __call__ = forward

    @torch.no_grad()
    def act(self, idx, do_sample=True, generator=None):
        """= GPT.act (model.py:244-260).  With a torch `generator` the draw is torch.multinomial on the
        device from OUR logits (same masking/softmax as the reference); without one the library's fused
        sampler runs, keyed by (seed drawn once from torch's global RNG, call counter, row) so that
        successive calls draw fresh uniforms like the reference's advancing global RNG does.
        Returns an int64 tensor [B] (0-d for B == 1, like the reference's .squeeze())."""
        tokens = self._tokens_u8(idx)
        if tokens.shape[1] != 256:                 # short rows (never the hot path): logits from the fp32 kernels, then the reference's own call shape
            logits = self.logits_tokens_t(tokens)
            if do_sample:
                return torch.multinomial(torch.softmax(logits[:, :5], dim=-1), num_samples=1, generator=generator).squeeze()   # model.py:250-257
            return torch.argmax(logits[:, :5], dim=-1).squeeze()                                                               # model.py:258-259
        if do_sample and generator is not None:
            logits = self.logits_tokens(tokens)
            probs = torch.softmax(logits[:, :5], dim=-1)                       # model.py:250-254
            nxt = torch.multinomial(probs, num_samples=1, generator=generator)  # model.py:257
            return nxt.squeeze()
        if do_sample:
            # The library sampler's seed is drawn from torch's global (CPU) RNG at the first SAMPLED call (a greedy first call
            # must not pin seed 0) and drawn again -- call counter back to 0 -- whenever that RNG was touched since our draw:
            # torch.manual_seed(s), also with the SAME s as before (the usual reproducibility pattern: the second run then
            # replays the first one's draws, as the reference's multinomial would), or any other consumer of the global stream.
            # (A seed pinned with reset_sampler(seed) is kept until reset_sampler() is called again: no look at the global RNG --
            #  another thread's act() or any torch.manual_seed silently dropped the pin, and the 5-KB state snapshot of
            #  every call sat on the one-environment latency path.)
            pinned = getattr(self, "_act_pinned", False)
            if not pinned and (getattr(self, "_act_seed", None) is None or not torch.equal(torch.get_rng_state(), self._act_rng_after)):
                self._act_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                self._act_rng_after = torch.get_rng_state()
                self._act_calls = 0
        step = self._act_calls
        self._act_calls += 1
        return self.act_tokens(tokens, do_sample=do_sample, seed=getattr(self, "_act_seed", None) or 0, step=step).to(torch.int64).squeeze()

    def reset_sampler(self, seed=None):
        """Explicit control of the generator-less sampler: forget the drawn seed (the next sampled act() draws a new one from
        torch's global RNG) or pin `seed`; the call counter restarts either way."""
        self._act_calls = 0
        if seed is None:
            self._act_seed = None
            self._act_pinned = False
        else:
            self._act_seed = int(seed)
            self._act_pinned = True


    # ---- training (include/mapf_gpt_amd.h: mgpt_gpt_train_alloc & co.; exact fp32) ------------------------------------
    def named_parameters(self):
        """(name, shape) of the parameters in model.py's named_parameters order (lm_head.weight is transformer.wte.weight, counted once)."""
        c = self.config
        C, L = c.n_embd, c.n_layer
        out = [("transformer.wte.weight", (c.vocab_size, C)), ("transformer.wpe.weight", (c.block_size, C))]
        for l in range(L):
            p = f"transformer.h.{l}."
            out += [(p + "ln_1.weight", (C,)), (p + "attn.c_attn.weight", (3 * C, C)), (p + "attn.c_proj.weight", (C, C)),
                    (p + "ln_2.weight", (C,)), (p + "mlp.c_fc.weight", (4 * C, C)), (p + "mlp.c_proj.weight", (C, 4 * C))]
        out.append(("transformer.ln_f.weight", (C,)))
        return out

    def train(self, mode=True, max_rows=None):
        """mode=True: training mode.  The first call allocates the training workspace (max_rows rows per chunk, default: the model's max_rows)
        with zeroed gradients and AdamW moments.  Later calls keep it: train() with no max_rows changes nothing (train.py calls model.train()
        after every evaluation), a different max_rows re-sizes the activation part only -- gradients, moments and step counts survive.
        train(False) = eval() and keeps the workspace.  bias=False and block_size 256 only.  config.dropout > 0: forward_backward drops as
        model.py does in training mode, with masks of the stream set_dropout_rng(seed) pinned; after eval() it runs without dropout, as
        torch does.  The masks are a counter hash with no generator behind it, so there is no default seed: train() of a dropout > 0 config
        before set_dropout_rng raises NotImplementedError, as it did when dropout was not built."""
        if not mode:
            return self.eval()
        assert self._loaded, "load_state_dict first"
        if self.config.dropout > 0 and getattr(self, "_drop_seed", None) is None:
            raise NotImplementedError("training with dropout > 0 draws its masks from a counter hash keyed by a seed, and no default seed is "
                                      "implemented: call set_dropout_rng(seed) before train()")
        have = getattr(self, "_train_rows", None)
        rows = int(max_rows) if max_rows is not None else (have or self.max_rows)
        if have != rows:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mgpt_gpt_train_alloc(self._h, rows))
            self._train_rows = rows
        self.training = True
        return self

    def _require_train(self):
        if getattr(self, "_train_rows", None) is None:
            raise RuntimeError("call train() first: it allocates the training workspace")

    def set_dropout_rng(self, seed, step=0):
        """Pin the dropout masks of forward_backward: mask = f(seed, step, site, layer, element) (sampling.dropout_keep), a counter hash as the
        action sampler's.  forward_backward uses `step` and increments it per call.  A dropout > 0 config needs this call before train()."""
        self._drop_seed, self._drop_step = int(seed), int(step)

    def forward_backward(self, idx, targets, loss_scale=1.0, precision="f32", *, dropout_step=None, row0=0, dropout_sites=15):
        """= loss = model(idx, targets)[1]; (loss * loss_scale).backward() (model.py:180-184, train.py:324-331): gradients ACCUMULATE into the
        device buffer; returns the unscaled mean cross-entropy (ignore_index=-1) as a 0-d float32 device tensor.  precision "f32": exact fp32;
        "bf16": train.py's torch.amp.autocast(bfloat16) regime (bf16 MFMA linears, fp32 gradients and master weights).  Micro-steps of
        either precision accumulate into the same buffer.
        In training mode a config.dropout > 0 drops at model.py's four places (:129/:175, :59/:66, :71, :88) with masks keyed by
        (set_dropout_rng's seed, step, row0 + row): dropout_step overrides the call counter and does not increment it, row0 is the global
        index of the call's first row (so a batch split over calls draws the masks of the whole batch), dropout_sites a bit mask of the four
        places (15 = all; tests name one).  After eval() / train(False) the call runs without dropout."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self._require_train()
        tokens = self._tokens_u8(idx)
        B, T = tokens.shape
        targets = torch.as_tensor(targets)
        if targets.dtype.is_floating_point or targets.dtype == torch.bool or targets.numel() != B * T:
            raise ValueError(f"targets must be an integer tensor of {B * T} elements (idx is {B} x {T}), got {targets.dtype} {tuple(targets.shape)}")
        tg = targets.reshape(B, T).to(device=self.device, dtype=torch.int32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        p = float(self.config.dropout) if self.training else 0.0
        step = dropout_step
        if step is None:
            step = getattr(self, "_drop_step", 0)
            if p > 0:
                self._drop_step = step + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_forward_backward_drop(self._h, _lib.ptr(tokens), B, T, _lib.ptr(tg), float(loss_scale), _lib.ptr(loss),
                                                                 _lib.PRECISIONS[precision], p, (getattr(self, "_drop_seed", None) or 0) & 0xFFFFFFFFFFFFFFFF,
                                                                 int(step) & 0xFFFFFFFFFFFFFFFF, int(row0), int(dropout_sites), _lib.stream_ptr()))
        return loss

    def forward_backward_rows(self, rows_u8, labels, loss_scale=1.0, precision="f32", check=True):
        """forward_backward for rows with ONE targeted position, token 255 (what dataset_rows, EpisodeStore, the .arrow shards and
        ArrowBatches(labels=True) carry): = forward_backward(rows_u8, targets) with targets[r, 255] = labels[r] and -1 elsewhere, the loss
        the mean over the call's rows.  rows_u8 int8 / uint8 [B, 256] and labels (any integer dtype, [B]) may live on the host or the
        device; casts happen on the device and no [B, 256] target matrix is built.  The last layer, ln_f, the head and the cross-entropy run
        on token 255 only, and the call never waits for the device (the general call waits once per call for its targeted-position count).
        check=True validates the labels against [0, 67) with one min / max (a wait when they live on the device); with check=False an
        out-of-range label makes the loss and the next gradient norm NaN.  Gradients accumulate into the same buffer as forward_backward's,
        in either precision.  This call has no dropout: a config.dropout > 0 in training mode raises NotImplementedError
        (forward_backward_rows_drop and forward_backward serve it); after eval() the call runs, as the general one does."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self._require_train()
        if self.training and self.config.dropout > 0:
            raise NotImplementedError(f"forward_backward_rows has no dropout (config.dropout = {self.config.dropout}): use "
                                      "forward_backward(idx, targets), the general call, which serves it")
        return self._rows_call(rows_u8, labels, loss_scale, precision, check, 0.0, 0, 0, 0)

    def forward_backward_rows_drop(self, rows_u8, labels, loss_scale=1.0, precision="f32", check=True, *, dropout_step=None, row0=0,
                                   dropout_sites=15):
        """forward_backward_rows with forward_backward's dropout: = forward_backward(rows_u8, targets, ..., dropout_step=, row0=,
        dropout_sites=) with targets[r, 255] = labels[r] and -1 elsewhere -- the same masks (the compact last layer draws the general
        call's at token / query 255), the same step counter (set_dropout_rng; incremented per call when p > 0; dropout_step overrides it
        without incrementing it), p = config.dropout in training mode and 0 after eval(), where the call is forward_backward_rows.
        rows_u8, labels and check as forward_backward_rows takes them; no host wait."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self._require_train()
        p = float(self.config.dropout) if self.training else 0.0
        return self._rows_call(rows_u8, labels, loss_scale, precision, check, p, dropout_step, row0, dropout_sites)

    def _rows_call(self, rows_u8, labels, loss_scale, precision, check, p, step, row0, sites):
        tokens = self._tokens_u8(rows_u8)
        B, T = tokens.shape
        if T != 256:
            raise ValueError(f"rows_u8 must be [B, 256], got {tuple(tokens.shape)}")
        labels = torch.as_tensor(labels)
        if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dim() != 1 or labels.numel() != B:
            raise ValueError(f"labels must be an integer tensor [{B}] (one per row), got {labels.dtype} {tuple(labels.shape)}")
        if check and B and (int(labels.min()) < 0 or int(labels.max()) >= 67):
            raise ValueError("labels must lie in [0, 67)")
        lb = labels.to(device=self.device, dtype=torch.int32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        if step is None:
            step = getattr(self, "_drop_step", 0)
            if p > 0:
                self._drop_step = step + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_forward_backward_rows_drop(self._h, _lib.ptr(tokens), B, _lib.ptr(lb), float(loss_scale), _lib.ptr(loss),
                                                                      _lib.PRECISIONS[precision], p, (getattr(self, "_drop_seed", None) or 0) & 0xFFFFFFFFFFFFFFFF,
                                                                      int(step) & 0xFFFFFFFFFFFFFFFF, int(row0), int(sites), _lib.stream_ptr()))
        return loss

    def zero_grad(self, set_to_none=True):
        self._require_train()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_zero_grad(self._h, _lib.stream_ptr()))

    def clip_grad_norm_(self, max_norm):
        """= torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm); returns the total norm as a 0-d device tensor (max_norm <= 0: norm only)."""
        self._require_train()
        total = torch.empty((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_clip_grad_norm(self._h, float(max_norm), _lib.ptr(total), _lib.stream_ptr()))
        return total

    def _train_tensor(self, name, which, shape):
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_train_get(self._h, name.encode(), which, _lib.ptr(out), out.numel(), _lib.stream_ptr()))
        return out

    def _set_train_tensor(self, name, which, value):
        a = torch.as_tensor(value).detach().to(device=self.device, dtype=torch.float32).contiguous()
        torch.cuda.synchronize(self.device)
        _lib.check(_lib.lib().mgpt_gpt_train_set(self._h, name.encode(), which, _lib.ptr(a), a.numel(), 1))

    def grads(self):
        """{named_parameters name: float32 device tensor} -- copies of the accumulated gradients."""
        self._require_train()
        return {n: self._train_tensor(n, _lib.TRAIN_GRAD, shp) for n, shp in self.named_parameters()}

    # ---- data-parallel gradient synchronisation (train.py:237-239, 314-322; training.py runs it between all_gather and the clip) ----
    def grads_size(self):
        """Length of the flat gradient buffer (the library's layout: every parameter once, any padding included)."""
        self._require_train()
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().mgpt_gpt_grads_size(self._h, ctypes.byref(n)))
        return int(n.value)

    def export_grads(self, out=None):
        """The whole gradient buffer as one flat float32 device tensor (a copy on the current stream), into `out` when given."""
        n = self.grads_size()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != n:
            raise ValueError(f"out must be a contiguous float32 device tensor of {n} elements, got {out.dtype} {tuple(out.shape)} on {out.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_grads_export(self._h, _lib.ptr(out), out.numel(), _lib.stream_ptr()))
        return out

    def reduce_grads(self, gathered, scale):
        """gathered float32 device [world, grads_size()] = the ranks' export_grads() in rank order: REPLACES the gradients with
        scale * (((g[0] + g[1]) + g[2]) + ...), fp32 additions in rank order (bit-identical on every rank); scale = 1 / world is DDP's mean."""
        n = self.grads_size()
        gathered = torch.as_tensor(gathered)
        if gathered.dtype != torch.float32 or not gathered.is_cuda or gathered.numel() % n != 0:
            raise ValueError(f"gathered must be a float32 device tensor of world x {n} elements, got {gathered.dtype} {tuple(gathered.shape)} "
                             f"on {gathered.device}")
        gathered = gathered.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_gpt_grads_reduce(self._h, _lib.ptr(gathered), gathered.numel() // n, float(scale), _lib.stream_ptr()))

    def state_dict(self):
        """The parameters read back from the device, in the reference's key layout; lm_head.weight aliases transformer.wte.weight."""
        assert self._loaded, "load_state_dict first"
        if self.config.bias:
            raise NotImplementedError("state_dict() reads the weights of bias=False models (the bias vectors have no read-back)")
        sd = {n: self._train_tensor(n, _lib.TRAIN_PARAM, shp) for n, shp in self.named_parameters()}     # (needs no training workspace)
        sd["lm_head.weight"] = sd["transformer.wte.weight"]
        return sd

    def configure_optimizers(self, weight_decay, learning_rate, betas, device_type="cuda"):
        """= GPT.configure_optimizers (model.py:202-226): AdamW with weight decay on the tensors of dim >= 2 only."""
        self._require_train()
        return AdamW(self, learning_rate, betas, weight_decay)


class AdamW:
    """torch.optim.AdamW over a GPT's device parameters (mgpt_gpt_adamw_step), with nanoGPT's two groups (model.py:209-214): group 0 the
    tensors of dim >= 2 (weight_decay), group 1 the LayerNorm gains (0).  param_groups[i]["lr"] may be set between steps, as train.py:282-283
    does; both groups take group 0's lr, betas and eps.  state_dict() / load_state_dict() use torch.optim.AdamW.state_dict()'s layout."""

    def __init__(self, net, lr, betas, weight_decay, eps=1e-8):
        self.net = net
        names = [n for n, _ in net.named_parameters()]
        shapes = dict(net.named_parameters())
        self._names = [n for n in names if len(shapes[n]) >= 2] + [n for n in names if len(shapes[n]) < 2]
        self._shapes = shapes
        n_decay = sum(len(shapes[n]) >= 2 for n in names)
        common = dict(lr=float(lr), betas=tuple(float(b) for b in betas), eps=float(eps), amsgrad=False, maximize=False, foreach=None,
                      capturable=False, differentiable=False, fused=None)
        self.param_groups = [dict(common, weight_decay=float(weight_decay), params=list(range(n_decay))),
                             dict(common, weight_decay=0.0, params=list(range(n_decay, len(self._names))))]

    def step(self):
        g = self.param_groups[0]
        if self.param_groups[1]["lr"] != g["lr"]:
            raise ValueError("both parameter groups must share one learning rate (train.py:282-283 sets it on every group)")
        with torch.cuda.device(self.net.device):
            _lib.check(_lib.lib().mgpt_gpt_adamw_step(self.net._h, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                                      _lib.stream_ptr()))

    def zero_grad(self, set_to_none=True):
        self.net.zero_grad()

    def state_dict(self):
        state = {}
        for i, n in enumerate(self._names):
            shp = self._shapes[n]
            step = self.net._train_tensor(n, _lib.TRAIN_STEP, (1,))
            if float(step.item()) == 0.0:
                continue                      # torch keeps no state for a parameter that never stepped
            state[i] = {"step": step.reshape(()).cpu(), "exp_avg": self.net._train_tensor(n, _lib.TRAIN_EXP_AVG, shp),
                        "exp_avg_sq": self.net._train_tensor(n, _lib.TRAIN_EXP_AVG_SQ, shp)}
        groups = [{k: (list(v) if k == "params" else v) for k, v in grp.items()} for grp in self.param_groups]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        for mine, theirs in zip(self.param_groups, groups):
            for k in ("lr", "betas", "eps", "weight_decay"):
                mine[k] = tuple(theirs[k]) if k == "betas" else theirs[k]
        order = [i for grp in groups for i in grp["params"]]
        for pos, i in enumerate(order):
            n = self._names[pos]
            st = sd["state"].get(i)
            if st is None:
                st = {"step": 0.0, "exp_avg": torch.zeros(self._shapes[n]), "exp_avg_sq": torch.zeros(self._shapes[n])}
            self.net._set_train_tensor(n, _lib.TRAIN_STEP, torch.as_tensor(float(st["step"])).reshape(1))
            self.net._set_train_tensor(n, _lib.TRAIN_EXP_AVG, st["exp_avg"])
            self.net._set_train_tensor(n, _lib.TRAIN_EXP_AVG_SQ, st["exp_avg_sq"])


def build_model(name_or_args, seed=0, scale=1.0, max_rows=2048, precision="f32", device="cuda", state_dict=None, envelope="fallback"):
    """Convenience: GPT with the named shape ("2M", "6M", "85M", "tiny") and synthetic or given weights."""
    args = weights.model_args(name_or_args)
    net = GPT(GPTConfig(**args), max_rows=max_rows, precision=precision, device=device, envelope=envelope)
    net.load_state_dict(state_dict if state_dict is not None else weights.synthetic_state_dict(args, seed=seed, scale=scale))
    return net.eval()
