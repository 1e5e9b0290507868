"""Host side of the HIP path: ROI tables resident in HBM, job descriptors, launches.

A *job* is one independent model of the sweep (a (fold, procedure) cell): its packed ROI
tables, flat fp32 parameters, Adam moments and workspace.  A *JobSet* is the device array
of descriptors one kernel launch runs -- one workgroup per job.
PyTorch is used for device memory and streams only; all arithmetic is in libnmhip.so.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import zlib
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .layout import ModelSpec, ParamLayout, rowsplit_limit

BATCH = _lib.NM_BATCH

# nm_devpass_multi as the automatic pick of JobSet.forward(loss=False), per number of experts: on only where the compact
# kernel's slowest repeat beat the general kernel's fastest at every set size measured (tools/bench_devpass_multi.py,
# profiles/devpass_multi.json)
DEVPASS_MULTI_AUTO = {2: True, 3: True, 4: True}

# nm_latent_pass as the automatic pick of JobSet.latent(), per number of experts: on only where the encoder-only kernel's
# slowest repeat beat the general forward kernel's fastest at every set size measured (tools/bench_latent.py,
# profiles/latent_pass.json).  Two experts: the record holds no set of that class yet, so the class
# stays on the general kernel until it does (JobSet.latent(compact=True) reaches nm_latent_pass all the same)
LATENT_AUTO = {1: True, 2: False, 3: True, 4: True}

# nm_decode_pass as the automatic route of the drop-in classes' decode(z, c, m), per number of decoders of the model: on only
# where the decoder-only kernel's slowest repeat beat the fastest of today's route (the one-modality copy on the general
# kernel with NM_F_ZGIVEN) at every set size measured (tools/bench_decode.py, profiles/decode_pass.json, DESIGN.md section
# 4b).  The record times the grid workload (54 cells a launch), not single decode() calls: no class holds a record of those
# yet, so decode() reaches the pass with NMHIP_DECODE=1; decode_grid, normative_trajectory and pred_recon_counterfactual have
# no other route and take it wherever the job is admitted
DECODE_AUTO = {1: False, 2: False, 3: False, 4: False}

# nm_chart_pass as the automatic route of normative_trajectory, per number of decoders: by the same rule (the new route's
# slowest repeat against decode() + cohort_moments' fastest at every set size measured, tools/bench_chart.py,
# profiles/chart_pass.json).  All off: the route is reached with fold="kernel" or NMHIP_CHART=1
CHART_AUTO = {1: False, 2: False, 3: False, 4: False}

# nm_e2e_pass as the automatic route of JobSet.forward_endtoend (and of cVAE_multimodal_endtoend.predict), per number of
# experts of the model: by the same rule (the new kernel's slowest repeat against the fastest of forward + head_classifier +
# the torch fold at EVERY set size measured, tools/bench_endtoend_eval.py, profiles/endtoend_eval.json, DESIGN.md section
# 4b).  All off: three experts win from 1 to 20 models and with five folds in one launch, and lose with the logits alone at
# 256 models; the other classes have no record.  The route is reached with compact=True or NMHIP_E2E=1
E2E_AUTO = {1: False, 2: False, 3: False, 4: False}

# nm_fi_pass as the automatic route of JobSet.forward_fi, per number of experts of the model: by the same rule (the new
# kernel's slowest repeat against the fastest of the forward kernel + nm_head_regression per draw + the torch fold at EVERY set
# size measured, tools/bench_fi_eval.py, profiles/fi_eval.json).  All off: three experts win at every
# size with 32 draws, with five folds in one launch and at one model with one draw (161 against 270 us), but with one draw
# the pass loses to forward + head_regression on standing descriptors from five models on (302 against 284 us, 733 against
# 482 us at 20, 12.2 against 1.88 ms at 256: one workgroup per CU); the other classes have no record.  The route is reached with compact=True or NMHIP_FI=1
FI_AUTO = {1: False, 2: False, 3: False, 4: False}

_MASK64 = (1 << 64) - 1


def pack_covariates(c, Cz: int, rows_alloc: int, device) -> torch.Tensor:
    """Covariate rows c [R, C] -> the bf16 block [rows_alloc, Cz] the decoders read beside z: c | 1 | 0 per row, zero rows
    past R -- byte for byte what Table holds in .cz for the same c (the same float32 -> bf16 rounding)."""
    c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c)
    if c.dim() != 2:
        raise ValueError(f"covariates must be [rows, C], got {tuple(c.shape)}")
    R, Cc = int(c.shape[0]), int(c.shape[1])
    if Cc + 1 > Cz or Cz % 8 != 0 or R > rows_alloc:
        raise ValueError(f"covariates [{R}, {Cc}] do not fit a block of {rows_alloc} rows of pitch {Cz}")
    out = torch.zeros(rows_alloc, Cz, dtype=torch.bfloat16, device=device)
    if Cc:
        out[:R, :Cc] = c.to(device=device, dtype=torch.float32).to(torch.bfloat16)
    out[:R, Cc] = 1.0
    return out


def check_decode_request(n_rows: int, rows_alloc: int, n_cells: int, Z: int, Cz: int, pitches: Sequence[int], z, cgrid, cz, x,
                         loc, sqerr, rowdev):
    """The rules of an nm_decode_t the library cannot check (the request lives in device memory): raised here, before the
    upload.  pitches: x_pitch per decoder; z / cgrid: tensors or None; cz, x, loc, sqerr, rowdev: per decoder a tensor (its
    whole storage) or None.  Only sizes are read: the tensors may live anywhere."""
    if not 0 <= int(n_cells) <= _lib.NM_MAX_CELLS:
        raise ValueError(f"n_cells must be 0 to {_lib.NM_MAX_CELLS}, got {n_cells}")
    if n_rows < 1 or rows_alloc % BATCH != 0 or rows_alloc < n_rows:
        raise ValueError(f"rows_alloc must be a multiple of {BATCH} and at least n_rows >= 1, got {rows_alloc} for {n_rows} rows")
    if len(pitches) > _lib.NM_MAX_EXP:
        raise ValueError(f"a request holds at most {_lib.NM_MAX_EXP} decoders, got {len(pitches)}")
    if z is None or z.numel() < rows_alloc * Z:
        raise ValueError(f"z must hold [{rows_alloc}, {Z}] values")
    cells = max(int(n_cells), 1)
    if n_cells > 0 and (cgrid is None or cgrid.numel() < n_cells * Cz):
        raise ValueError(f"c_grid must hold [{n_cells}, {Cz}] packed values")
    if not any(t is not None for t in loc):
        raise ValueError("no decoder is wanted: every loc is None")
    for m, xp in enumerate(pitches):
        if loc[m] is None:
            if sqerr[m] is not None or rowdev[m] is not None:
                raise ValueError(f"decoder {m}: sqerr / rowdev without loc (a decoder without loc is skipped)")
            continue
        if n_cells == 0 and (cz[m] is None or cz[m].numel() < rows_alloc * Cz):
            raise ValueError(f"decoder {m}: per-row covariates must hold [{rows_alloc}, {Cz}] packed values")
        if (sqerr[m] is not None or rowdev[m] is not None) and x[m] is None:
            raise ValueError(f"decoder {m}: sqerr / rowdev are taken against x, which is not given")
        if x[m] is not None and x[m].numel() < rows_alloc * xp:
            raise ValueError(f"decoder {m}: x must hold [{rows_alloc}, {xp}] values")
        for what, t, need in (("loc", loc[m], cells * rows_alloc * xp), ("sqerr", sqerr[m], cells * rows_alloc * xp),
                              ("rowdev", rowdev[m], cells * rows_alloc)):
            if t is not None and t.numel() < need:
                raise ValueError(f"decoder {m}: {what} holds {t.numel()} values, its declared shape needs {need}")


def check_chart_request(n_rows: int, rows_alloc: int, n_cells: int, Z: int, Cz: int, pitches: Sequence[int], z, cgrid, part,
                        chart, loc):
    """The rules of an nm_chart_t the library cannot check (the request lives in device memory): raised here, before the
    upload, as check_decode_request does for nm_decode_t.  part, chart, loc: per decoder a tensor (its whole storage) or
    None.  Only sizes are read."""
    if not 1 <= int(n_cells) <= _lib.NM_MAX_CELLS:
        raise ValueError(f"n_cells must be 1 to {_lib.NM_MAX_CELLS} (a chart needs a grid), got {n_cells}")
    if n_rows < 1 or n_rows > _lib.NM_CHART_MAX_ROWS or rows_alloc % BATCH != 0 or rows_alloc < n_rows:
        raise ValueError(f"rows_alloc must be a multiple of {BATCH} and at least n_rows (1 to {_lib.NM_CHART_MAX_ROWS}), "
                         f"got {rows_alloc} for {n_rows} rows")
    if len(pitches) > _lib.NM_MAX_EXP:
        raise ValueError(f"a request holds at most {_lib.NM_MAX_EXP} decoders, got {len(pitches)}")
    if z is None or z.numel() < rows_alloc * Z:
        raise ValueError(f"z must hold [{rows_alloc}, {Z}] values")
    if cgrid is None or cgrid.numel() < n_cells * Cz:
        raise ValueError(f"c_grid must hold [{n_cells}, {Cz}] packed values")
    if not any(t is not None for t in part) and not any(t is not None for t in loc):
        raise ValueError("no decoder is wanted: every part and every loc is None")
    for m, xp in enumerate(pitches):
        if chart[m] is not None and part[m] is None:
            raise ValueError(f"decoder {m}: chart without part (the merge reads the tile partials)")
        if part[m] is not None and chart[m] is None:
            raise ValueError(f"decoder {m}: part without chart")
        for what, t, need in (("part", part[m], n_cells * (rows_alloc // 128) * xp * 2),
                              ("chart", chart[m], n_cells * xp * _lib.NM_CHART_COLUMNS), ("loc", loc[m], n_cells * rows_alloc * xp)):
            if t is not None and t.numel() < need:
                raise ValueError(f"decoder {m}: {what} holds {t.numel()} values, its declared shape needs {need}")


def draw_seeds(seed: int, n_draws: int) -> List[int]:
    """The default generator keys of the posterior-predictive pass: draw 0 is the job's own seed (S = 1 is the parity pass),
    draw s is (seed + s * 0x9E3779B97F4A7C15) mod 2^64 -- the golden-ratio stride keeps the keys of neighbouring seeds apart."""
    return [(int(seed) + s * 0x9E3779B97F4A7C15) & _MASK64 for s in range(int(n_draws))]


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device) -> int:
    """The current HIP stream of `device` as an integer handle.  (torch.cuda.current_stream() builds a Stream object --
    ~6 us a call, eight calls per step of the eager classes; the raw getter is what torch.cuda's own internals use.)"""
    if _RAW_STREAM is not None:
        d = torch.device(device)
        return int(_RAW_STREAM(d.index if d.index is not None else torch.cuda.current_device()))
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.NmError("no HIP device visible: the cVAE hot path runs on MI355X only (no CPU fallback)")
    return torch.device(device if device is not None else "cuda:0")


class Table:
    """One modality's ROI table in HBM.

    ``x`` [N, D] and covariates ``c`` [N, C] (any float/int dtype; the reference's
    ``torch.cat((x, c))`` promotes to float32, cVAE.py:163) become
      x_f32 [rows_alloc, x_pitch] fp32, zero rows beyond N, pitch = D rounded up to 4 (residual / NLL side)
      xb    [rows_alloc, Kx] bf16  x | c | 1 | 0             (MFMA operand side)
    with rows_alloc a multiple of 256 and Kx a multiple of 32.
    """

    def __init__(self, x, c, device=None):
        dev = require_gpu(device)
        lib = _lib.load()
        # content key of the covariates: tables with equal keys carry the same covariate block, which lets the
        # decoders of a model share one z | c | 1 input (nm_job_t.shared_cov).  Host data: shape, dtype and two
        # checksums of the bytes; device tensors: identity of the storage (no device-to-host copy, no sync)
        if torch.is_tensor(c) and c.is_cuda:
            self.c_key = ("dev", c.data_ptr(), tuple(c.shape), str(c.dtype), c._version)
            self._keep = (c,)            # the key is the storage's identity: the storage must outlive the table
        else:
            c_host = c.detach().contiguous().numpy() if torch.is_tensor(c) else np.ascontiguousarray(np.asarray(c))
            self.c_key = (tuple(c_host.shape), str(c_host.dtype), zlib.crc32(c_host.tobytes()), zlib.adler32(c_host.tobytes()))
        x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
        c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c)
        if x.dim() != 2 or c.dim() != 2 or x.shape[0] != c.shape[0]:
            raise ValueError(f"x must be [N, D] and c [N, C] with equal N, got {tuple(x.shape)} / {tuple(c.shape)}")
        self.N, self.D = int(x.shape[0]), int(x.shape[1])
        self.C = int(c.shape[1])
        self.rows_alloc = max(1, math.ceil(self.N / BATCH)) * BATCH
        self.Kx = (self.D + self.C + 1 + 31) // 32 * 32
        self.Cz = (self.C + 1 + 7) // 8 * 8
        xs = x.to(device=dev, dtype=torch.float32).contiguous()
        cs = c.to(device=dev, dtype=torch.float32).contiguous()
        self.x_pitch = (self.D + 3) // 4 * 4
        self.x_f32 = torch.empty(self.rows_alloc, self.x_pitch, dtype=torch.float32, device=dev)
        # xb: 64-column chunk images of 256-row tiles, [tiles][chunks][256][72] (nm_modality_t.xb)
        self.xb = torch.empty(int(lib.nm_xb_elems(self.rows_alloc, self.Kx)), dtype=torch.bfloat16, device=dev)
        self.cz = torch.empty(self.rows_alloc, self.Cz, dtype=torch.bfloat16, device=dev)
        _lib.check(lib.nm_pack_table(xs.data_ptr(), cs.data_ptr() if self.C > 0 else None, self.N, self.rows_alloc,
                                     self.D, self.C, self.Kx, self.xb.data_ptr(), self.x_f32.data_ptr(),
                                     self.x_pitch, self.cz.data_ptr(), self.Cz, _stream_ptr(dev)), "nm_pack_table")
        self.device = dev

    def repack(self, x, c) -> bool:
        """Overwrite this table's contents with a new batch of the same shape (the eager facade calls the model once per
        batch: the buffers, and with them the job descriptor, stay as they are).  False if the shapes differ."""
        if not (torch.is_tensor(x) and torch.is_tensor(c)) or x.dim() != 2 or c.dim() != 2:
            return False
        if int(x.shape[0]) != self.N or int(x.shape[1]) != self.D or int(c.shape[1]) != self.C or int(c.shape[0]) != self.N:
            return False
        lib = _lib.load()
        dev = self.device
        self.c_key = (("dev", c.data_ptr(), tuple(c.shape), str(c.dtype), c._version) if c.is_cuda else
                      ("host", id(c), tuple(c.shape), str(c.dtype), c._version))
        xs = x.to(device=dev, dtype=torch.float32).contiguous()
        cs = c.to(device=dev, dtype=torch.float32).contiguous()
        self._keep = (c, xs, cs)
        _lib.check(lib.nm_pack_table(xs.data_ptr(), cs.data_ptr() if self.C > 0 else None, self.N, self.rows_alloc,
                                     self.D, self.C, self.Kx, self.xb.data_ptr(), self.x_f32.data_ptr(),
                                     self.x_pitch, self.cz.data_ptr(), self.Cz, _stream_ptr(dev)), "nm_pack_table")
        return True

    def packed_rows(self) -> torch.Tensor:
        """The packed operand rows x | c | 1 | 0 as a [rows_alloc, Kx] tensor (diagnostics / tests)."""
        nch = (self.Kx + 63) // 64
        t = self.xb.view(self.rows_alloc // BATCH, nch, BATCH, 72)[..., :64]
        return t.permute(0, 2, 1, 3).reshape(self.rows_alloc, nch * 64)[:, :self.Kx]

    @property
    def n_tiles(self) -> int:
        return self.rows_alloc // BATCH


class Job:
    """Parameters + optimizer state + tables of one model."""

    def __init__(self, spec: ModelSpec, tables: Sequence[Table], combine: str = "poe", state: Optional[Dict] = None,
                 lr: float = 1e-4, betas=(0.9, 0.999), adam_eps: float = 1e-8, kl_weight: Optional[float] = None,
                 ll_weight: float = 1.0, seed: int = 0, loss_cap: int = 1024, single_bypass: bool = True,
                 init_seed: int = 42, n_tiles_ws: int = 1):
        self.layout = ParamLayout(spec)
        self.spec = spec
        if len(tables) != spec.M:
            raise ValueError(f"need {spec.M} tables, got {len(tables)}")
        for m, t in enumerate(tables):
            if t.D != spec.input_dims[m] or t.C != spec.net_c_dim:
                raise ValueError(f"table {m}: D={t.D}, C={t.C} do not match the model ({spec.input_dims[m]}, {spec.net_c_dim})")
            if t.N != tables[0].N:
                raise ValueError("all modalities must hold the same subjects (rows)")
        combine_l = combine.lower()
        if combine_l not in _lib.NM_COMBINE:
            raise ValueError("No such combination method")            # cVAE.py:1163
        self.combine = combine_l
        self.tables = list(tables)
        dev = tables[0].device
        self.device = dev
        if state is None:
            state = self.layout.init_reference_rule(init_seed)
        self.params = self.layout.flatten(state, device=dev)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        self.lr, self.betas, self.adam_eps = float(lr), (float(betas[0]), float(betas[1])), float(adam_eps)
        # cVAE_multimodal adds KL once per modality (cVAE.py:1189-1195); class cVAE once (cVAE.py:497-500); the DMVAE
        # family: once per modality times beta (1.0, mmVAEPlus 0.05; cVAE.py:1507, 1911, 1570)
        dm_beta = {"dmvae": 1.0, "weighted_dmvae": 1.0, "mmvaeplus": 0.05}.get(spec.kind, 1.0)
        self.kl_weight = float(spec.M * dm_beta if kl_weight is None else kl_weight)
        if spec.is_dm:
            single_bypass = False                     # ProductOfExperts2 is always evaluated (cVAE.py:1547)
        # mvtCAE (cVAE.py:1754-1893): no single-expert bypass, 'poe' = ProductOfExperts2 fed with variances, joint variance
        # clamped at 1e-6, total = sum_i [kl + 1e-5 ll_i + beta tc] with beta = 1e-4 (the log-likelihood enters with a PLUS)
        self.var_floor, self.tc_weight = 0.0, 0.0
        if spec.kind == "mvtcae":
            single_bypass = False
            self.var_floor, self.tc_weight = 1e-6, spec.M * 1e-4
            if combine.lower() == "poe":
                self.combine = "poe2v"
            if ll_weight == 1.0:
                ll_weight = -1e-5
        self.kmods = spec.kernel_modalities()         # decoders the kernel runs: (table, has_encoder, prefix)
        self.dz_extra: Optional[torch.Tensor] = None  # d L_extra / d z          [rows_alloc, Z]
        self.dloc_extra: List[Optional[torch.Tensor]] = [None] * len(self.kmods)   # d L_extra / d x_hat [rows_alloc, x_pitch]
        self.ll_weight = float(ll_weight)
        # classifier head (kind == "endtoend" with classifier_layers)
        self.dloc_rowcoef: List[Optional[torch.Tensor]] = [None] * len(self.kmods)      # hinge row coefficients [rows_alloc]
        self.labels: Optional[torch.Tensor] = None    # int32 [rows_alloc]
        self.out_logits: Optional[torch.Tensor] = None
        self.cls_train, self.cls_use_mu = True, False
        self.cls_dropout, self.cls_margin, self.cls_w_ce, self.cls_w_contrast = 0.0, 1.0, 1.0, 0.1
        self.dephase_sleeps = 0          # set by JobSet (see nm_job_t.dephase)
        self.reg_lambda = 1.0                         # regression head (kind == "regression")
        self.fi_target: Optional[torch.Tensor] = None # [rows_alloc]
        self.out_fi_pred: Optional[torch.Tensor] = None
        self.reg_resid: Optional[torch.Tensor] = None # bf16 residual chunk images (nm_job_t.reg_resid)
        self.reg_dres: Optional[torch.Tensor] = None  # bf16 d MSE / d x_hat chunk images of the batch in flight
        self.single_bypass = bool(single_bypass)
        self.seed = int(seed)
        self.t = 0                       # optimizer steps taken
        self.step = 0                    # data steps taken (selects the batch)
        self.loss_cap = int(loss_cap)
        self.loss_log = torch.zeros(self.loss_cap, _lib.NM_LOSS_STRIDE, dtype=torch.float32, device=dev)
        self.eps: Optional[torch.Tensor] = None
        self.eps_cap = 1
        self.lr_table: Optional[torch.Tensor] = None   # fp64 [n]: learning rate of optimizer step t = lr_table[(t - 1) % n]
        self._ws = None
        self._ws_tiles = 0
        self._version = 0                # bumped whenever the descriptor would change
        self._wsh = None                 # bf16 shadow images of the weights (nm_job_t.wsh)
        self._gpart = None               # row-split launch: k slices of fp32 gradient partials (nm_job_t.gpart)
        self._gpart_k = 0
        self._rs_ok_version = None       # _version at which nm_rowsplit_ok last accepted this job
        self._rs_limit = (None, None)    # (Kx of the kernel modalities, layout.rowsplit_limit of them)
        self.shadow_dirty = True         # params were written by the host: nm_sync_shadow before the next launch
        self._ensure_workspace(n_tiles_ws)
        # optional exports
        self.out_mu = self.out_logvar = self.out_z = None
        nk = len(self.kmods)
        self.out_loc: List[Optional[torch.Tensor]] = [None] * nk
        self.out_sqerr: List[Optional[torch.Tensor]] = [None] * nk
        self.out_rowdev: List[Optional[torch.Tensor]] = [None] * nk
        # the modality-subset pass (enable_subset_exports): the subsets, their expert masks, exports per (subset, modality)
        self.subsets = self.sub_masks = self.sub_decoders = None
        self.sub_loc = self.sub_sqerr = self.sub_rowdev = None
        # the posterior-predictive pass (enable_predictive_exports): draws per row, their keys / injected noise, exports per modality
        self.n_draws = self.pred_seeds = self.pred_eps = self.noise_var = None
        self.pred_mean = self.pred_var = self.pred_msq = self.pred_z = self.pred_rowdev = self.pred_rowz2 = None
        # the decoder pass (enable_decode_exports / set_decode_inputs): the request's rows and cells, its inputs and exports
        self.dec_rows = self.dec_rows_alloc = self.dec_cells = self.dec_decoders = self.dec_full = None
        self.dec_z = self.dec_cgrid = self.dec_cz = self.dec_x = self.dec_loc = self.dec_sqerr = self.dec_rowdev = None
        self._dec_epoch = 0              # bumped whenever the request would change
        # the chart pass (enable_chart_exports / set_chart_inputs): the request, its inputs, partials, chart and optional loc
        self.chart_rows = self.chart_rows_alloc = self.chart_cells = self.chart_decoders = self.chart_full = None
        self.chart_z = self.chart_cgrid = self.chart = self.chart_loc = None
        self._chart_epoch = 0
        # the likelihood pass (enable_likelihood_exports): draws per row, decoder mask, the row export and per-decoder terms
        self.iw_draws = self.iw_seeds = self.iw_eps = self.iw_mask = self.iw_row = self.iw_recon_ll = self.iw_noise_var = None
        self._params_epoch = 0           # bumped by every host-side write of the parameters (refresh_noise_var)
        self._nv_state = None

    # -- buffers -------------------------------------------------------------------------------
    def _ensure_workspace(self, n_tiles: int):
        if self._ws is not None and self._ws_tiles >= n_tiles:
            return
        lib = _lib.load()
        probe = _lib.NmJob()
        probe.M, probe.L, probe.Z = len(self.kmods), len(self.spec.hidden), self.spec.latent
        probe.C, probe.wide = self.spec.net_c_dim, int(self.spec.wide)
        for i, h in enumerate(self.spec.hidden):
            probe.H[i] = h
        probe.cls_layers, probe.cls_classes = len(self.spec.classifier_layers), (self.spec.num_classes if self.spec.classifier_layers else 0)
        for i, w in enumerate(self.spec.classifier_layers):      # (blocks wider than 128: the head's workspace is in tiles)
            probe.cls_width[i] = w
        probe.reg_head = 1 if self.spec.kind == "regression" else 0
        probe.M_enc = self.spec.M
        for k, (m, _, _) in enumerate(self.kmods):
            probe.mod[k].D = self.tables[m].D
            probe.mod[k].Kx = self.tables[m].Kx
        self.ws_bytes = int(lib.nm_workspace_bytes(C.byref(probe)))
        if self._wsh is None:
            if self.spec.wide and self.spec.kind != "regression":   # the general-shape path reads the fp32 master: no shadow images
                self._wsh = torch.zeros(256, dtype=torch.uint8, device=self.device)
            else:                                    # (general-shape regression model: the regressor's first-layer images only)
                nb = int(lib.nm_fill_shadow(C.byref(probe)))
                if nb < 0:
                    _lib.check(nb, "nm_fill_shadow")
                self._wsh = torch.zeros(nb, dtype=torch.uint8, device=self.device)
        self._ws = torch.zeros(self.ws_bytes * n_tiles, dtype=torch.uint8, device=self.device)
        self._ws_tiles = n_tiles
        self._version += 1

    @property
    def gpart_stride(self) -> int:
        return (int(self.params.numel()) + 255) // 256 * 256

    def _ensure_rowsplit(self, k: int):
        """Buffers of a row-split launch with k slices per (model, modality): k workspace tiles, k gradient-partial slices."""
        self._ensure_workspace(k)
        if self._gpart is None or self._gpart_k < k:
            self._gpart = torch.zeros(k * self.gpart_stride, dtype=torch.float32, device=self.device)
            self._gpart_k = k
            self._version += 1

    def devpass_ok(self) -> bool:
        """nm_devpass_ok for this job, plus: no latent exports asked for (the general forward kernel writes those)."""
        s = self.spec
        return (not s.wide and len(self.kmods) == 1 and s.M == 1 and self.single_bypass and s.n_private == 0 and not s.is_dm
                and self.tc_weight == 0.0 and s.kind != "weighted_dmvae" and s.hidden[0] <= 112 and (s.latent + 15) // 16 * 16 <= 32
                and self.out_mu is None and self.out_logvar is None and self.out_z is None)

    def devpass_multi_ok(self) -> bool:
        """nm_devpass_multi_ok for this job -- several experts, every modality with an encoder, no private latent /
        learnable weights / total correlation, Gaussian output, first hidden width <= 112, latent <= 32 -- plus: no latent
        exports asked for (the general forward kernel writes those)."""
        s = self.spec
        return (not s.wide and len(self.kmods) == s.M and 2 <= s.M <= _lib.NM_MAX_EXP and s.n_private == 0 and not s.is_dm
                and self.tc_weight == 0.0 and s.kind != "weighted_dmvae" and s.hidden[0] <= 112 and (s.latent + 15) // 16 * 16 <= 32
                and self.out_mu is None and self.out_logvar is None and self.out_z is None)

    def latent_ok(self) -> bool:
        """nm_latent_pass_ok for this job: 1..NM_MAX_EXP experts, every modality with an encoder, no private latent /
        learnable weights / total correlation, Gaussian output, first hidden width <= 112, latent <= 32.  (The latent exports
        are what the pass writes: they play no part here.)"""
        s = self.spec
        return (not s.wide and len(self.kmods) == s.M and 1 <= s.M <= _lib.NM_MAX_EXP and s.n_private == 0 and not s.is_dm
                and self.tc_weight == 0.0 and s.kind != "weighted_dmvae" and s.hidden[0] <= 112 and (s.latent + 15) // 16 * 16 <= 32)

    def rowsplit_ok(self) -> bool:
        """Can this model run row-split (nm_rowsplit_ok: plain cVAE / cVAE_multimodal-type models on the fused kernel whose
        modalities fit the Adam sweep's tables, layout.rowsplit_limit)?"""
        s = self.spec
        return (not s.wide and s.kind in ("single", "multimodal") and len(self.kmods) == s.M and s.M <= _lib.NM_MAX_EXP
                and self.tc_weight == 0.0 and self.rowsplit_limit() is None)

    def plain_ok(self) -> bool:
        """nm_plain_ok for this job, read off the job as devpass_ok is: a cVAE / cVAE_multimodal trunk on the fused kernel with
        nothing the step kernel's plain-training instantiation has folded away -- no head and none of its extra gradients, no
        export buffer.  (The kinds left out carry the rest: the DMVAE family's sigmoid output, private columns and learnable
        weights, mvtCAE's total correlation, the end-to-end model's decoder-only modalities.)"""
        s = self.spec
        return (not s.wide and s.kind in ("single", "multimodal") and len(self.kmods) == s.M and self.tc_weight == 0.0
                and self.dz_extra is None and all(t is None for t in self.dloc_extra) and all(t is None for t in self.dloc_rowcoef)
                and self.out_mu is None and self.out_logvar is None and self.out_z is None
                and all(t is None for t in self.out_loc) and all(t is None for t in self.out_sqerr)
                and all(t is None for t in self.out_rowdev))

    def rowsplit_limit(self) -> Optional[str]:
        """The row-split sweep table limit a modality of this model exceeds (layout.rowsplit_limit), or None."""
        kxs = tuple(self.tables[m].Kx for m, _, _ in self.kmods)
        if self._rs_limit[0] != kxs:                               # (asked on every train() call of a small set)
            self._rs_limit = (kxs, rowsplit_limit(self.spec, kxs))
        return self._rs_limit[1]

    def set_fi(self, fi):
        """Regression target per table row (FI, ..._regression.py:86-87); padded with zeros to rows_alloc."""
        ra = self.tables[0].rows_alloc
        f = torch.as_tensor(fi, dtype=torch.float32).reshape(-1)
        if f.numel() != self.tables[0].N:
            raise ValueError(f"fi has {f.numel()} values for {self.tables[0].N} table rows")
        self.fi_target = torch.zeros(ra, device=self.device)
        self.fi_target[: f.numel()] = f.to(self.device)
        self._version += 1

    def set_labels(self, labels):
        """Class label per table row (classifier head); padded with zeros to rows_alloc."""
        ra = self.tables[0].rows_alloc
        l = torch.as_tensor(labels).reshape(-1).to(torch.int32)
        if l.numel() != self.tables[0].N:
            raise ValueError(f"labels has {l.numel()} values for {self.tables[0].N} table rows")
        self.labels = torch.zeros(ra, dtype=torch.int32, device=self.device)
        self.labels[: l.numel()] = l.to(self.device)
        self._version += 1

    def prepare_classifier(self):
        """Buffers the end-to-end train loop needs: exports (latent, per-subject deviations, logits) and the
        slots the head's backward fills (d CE / d z, hinge row coefficients)."""
        if self.out_z is None or any(o is None for o in self.out_rowdev) or self.out_logits is None:
            self.enable_exports(loc=False, sqerr=False, rowdev=True, latent=True)
        ra = self.tables[0].rows_alloc
        if self.dz_extra is None:
            self.dz_extra = torch.zeros(ra, self.spec.latent, device=self.device)
            self._version += 1
        if any(d is None for d in self.dloc_rowcoef):
            self.dloc_rowcoef = [torch.zeros(ra, device=self.device) for _ in self.kmods]
            self._version += 1

    def prepare_regression(self):
        """Buffers the regression head needs: the residual chunk images the trunk exports for it (one set per 256-row
        tile of the table), the d MSE / d x_hat images it hands back (one set: the batch in flight), the predictions."""
        nq = sum((self.tables[m].D + 63) // 64 for m in range(self.spec.M))
        img = 256 * 72 * 2
        if self.reg_resid is None or self.reg_resid.numel() < self.tables[0].n_tiles * nq * img:
            self.reg_resid = torch.zeros(self.tables[0].n_tiles * nq * img, dtype=torch.uint8, device=self.device)
            self.reg_dres = torch.zeros(nq * img, dtype=torch.uint8, device=self.device)
            self._version += 1
        if self.out_fi_pred is None:
            self.out_fi_pred = torch.zeros(self.tables[0].rows_alloc, device=self.device)
            self._version += 1

    def touch(self):
        """Call after changing tables / step / t / hyper-parameters by hand: forces a descriptor re-upload."""
        self._version += 1

    def set_lr_table(self, lrs):
        """Per-step learning rates (optimizer step t, 1-based, runs at lrs[(t - 1) % len]): the schedules that really
        reach the optimizer in the reference (`param_group['lr'] = clr`, multimodal_kfold_cvae_nmmlp.py:376-381;
        prep.cyclic_lr builds that one).  None: the constant lr."""
        self.lr_table = None if lrs is None else torch.as_tensor(np.asarray(lrs, dtype=np.float64)).to(self.device).contiguous()
        self._version += 1

    def set_eps(self, eps: Optional[torch.Tensor]):
        """Explicit reparameterisation draws [n_steps, 256, Z] (parity mode); None = in-kernel generator."""
        self._version += 1
        if eps is None:
            self.eps, self.eps_cap = None, 1
            return
        e = torch.as_tensor(eps, dtype=torch.float32)
        if e.dim() == 2:
            e = e.unsqueeze(0)
        if e.shape[1] != BATCH or e.shape[2] != self.spec.latent:
            pad = torch.zeros(e.shape[0], BATCH, self.spec.latent, dtype=torch.float32)
            pad[:, :e.shape[1]] = e
            e = pad
        self.eps = e.to(self.device).contiguous()
        self.eps_cap = int(self.eps.shape[0])

    def enable_exports(self, loc=True, sqerr=True, rowdev=True, latent=True):
        ra = self.tables[0].rows_alloc
        Z = self.spec.latent
        self._version += 1
        if latent:
            self.out_mu = torch.zeros(ra, Z, device=self.device)
            self.out_logvar = torch.zeros(ra, Z, device=self.device)
            self.out_z = torch.zeros(ra, Z, device=self.device)
        if self.spec.kind == "regression":
            self.out_fi_pred = torch.zeros(ra, device=self.device)
        if self.spec.kind == "endtoend" and self.spec.classifier_layers:
            self.out_logits = torch.zeros(ra, _lib.NM_MAX_CLASSES, device=self.device)
        for j, (m, _, _) in enumerate(self.kmods):
            t = self.tables[m]
            # storage rows share the fp32 table's pitch (16-byte stores in the kernel); the views are [rows, D]
            self.out_loc[j] = torch.zeros(ra, t.x_pitch, device=self.device)[:, :t.D] if loc else None
            self.out_sqerr[j] = torch.zeros(ra, t.x_pitch, device=self.device)[:, :t.D] if sqerr else None
            self.out_rowdev[j] = torch.zeros(ra, device=self.device) if rowdev else None

    def enable_subset_exports(self, subsets, loc=True, sqerr=True, rowdev=True, decoders=None):
        """Buffers of the modality-subset pass (JobSet.forward_subsets, nm_devpass_subsets).  subsets: a list of 1 to 15
        tuples of expert indices, each the experts one entry fuses; decoders: per subset the modalities to decode (None:
        every one) -- a decoder left out of an entry is skipped by the kernel.  Afterwards sub_loc[s][m], sub_sqerr[s][m]
        ([rows_alloc, D] views) and sub_rowdev[s][m] ([rows_alloc]) hold entry s's exports of modality m, None where the
        decoder or the kind of export was not asked for.  Refused (ValueError): an empty subset, an index beyond the
        model's experts, the same subset twice, no subset or more than 15."""
        M = len(self.kmods)
        subsets = [tuple(int(i) for i in s) for s in subsets]
        if not 1 <= len(subsets) <= _lib.NM_MAX_SUBSETS:
            raise ValueError(f"need 1 to {_lib.NM_MAX_SUBSETS} subsets, got {len(subsets)}")
        masks = []
        for s in subsets:
            if not s:
                raise ValueError("an empty subset has no joint posterior (mask 0)")
            if any(i < 0 or i >= M or i >= _lib.NM_MAX_EXP for i in s):
                raise ValueError(f"subset {s}: the model has experts 0..{min(M, _lib.NM_MAX_EXP) - 1}")
            mask = 0
            for i in s:
                mask |= 1 << i
            if mask in masks:
                raise ValueError(f"subset {s} is listed twice")
            masks.append(mask)
        if decoders is None:
            decoders = [tuple(range(M))] * len(subsets)
        decoders = [tuple(int(m) for m in d) for d in decoders]
        if len(decoders) != len(subsets) or any(m < 0 or m >= M for d in decoders for m in d):
            raise ValueError(f"decoders: one list of modalities 0..{M - 1} per subset")
        ra = self.tables[0].rows_alloc
        self.subsets, self.sub_masks, self.sub_decoders = subsets, masks, decoders
        self.sub_loc, self.sub_sqerr, self.sub_rowdev = [], [], []
        for d in decoders:
            pitch = [self.tables[m].x_pitch for m, _, _ in self.kmods]
            width = [self.tables[m].D for m, _, _ in self.kmods]
            self.sub_loc.append([torch.zeros(ra, pitch[m], device=self.device)[:, :width[m]] if loc and m in d else None
                                 for m in range(M)])
            self.sub_sqerr.append([torch.zeros(ra, pitch[m], device=self.device)[:, :width[m]] if sqerr and m in d else None
                                   for m in range(M)])
            self.sub_rowdev.append([torch.zeros(ra, device=self.device) if rowdev and m in d else None for m in range(M)])
        self._version += 1

    def subset_structs(self, present=None):
        """This job's row of nm_devpass_subsets' table: one NmSubset per entry.  present: per entry a uint8 device tensor
        [rows_alloc] or None."""
        if getattr(self, "sub_masks", None) is None:
            raise ValueError("enable_subset_exports() first")
        out = []
        for s, mask in enumerate(self.sub_masks):
            e = _lib.NmSubset()
            e.mask = mask
            p = present[s] if present is not None else None
            e.present = p.data_ptr() if p is not None else None
            for m in range(len(self.kmods)):
                for field, bufs in (("out_loc", self.sub_loc), ("out_sqerr", self.sub_sqerr), ("out_rowdev", self.sub_rowdev)):
                    getattr(e, field)[m] = bufs[s][m].data_ptr() if bufs[s][m] is not None else None
            out.append(e)
        return out

    def draws_ok(self) -> bool:
        """nm_devpass_draws_ok for this job, read off the job as latent_ok is: 1..NM_MAX_EXP experts (one expert with the
        bypass on or off), every modality with an encoder, no private latent / learnable weights / total correlation,
        Gaussian output, first hidden width <= 112, latent <= 32."""
        return self.latent_ok()

    def _draw_request(self, n_draws, seeds, eps, most):
        """The draws of a request, checked: -> (S, one generator key per draw, the injected draws on the device or None)."""
        S = int(n_draws)
        if not 1 <= S <= most:
            raise ValueError(f"n_draws must be 1 to {most}, got {n_draws}")
        if seeds is not None and eps is not None:
            raise ValueError("give seeds or eps, not both: an injected draw has no generator key")
        if seeds is not None and len(seeds) != S:
            raise ValueError(f"seeds: one per draw ({S}), got {len(seeds)}")
        if eps is not None and len(eps) != S:
            raise ValueError(f"eps: one tensor per draw ({S}), got {len(eps)}")
        keys = [int(v) & _MASK64 for v in seeds] if seeds is not None else draw_seeds(self.seed, S)
        if eps is None:
            return S, keys, None
        Z, out = self.spec.latent, []
        for e in eps:
            e = torch.as_tensor(e, dtype=torch.float32)
            if e.dim() == 2:
                e = e.unsqueeze(0)
            if e.dim() != 3 or e.shape[2] != Z or e.shape[1] > BATCH:
                raise ValueError(f"eps: every draw is [steps, <= {BATCH}, {Z}], got {tuple(e.shape)}")
            steps = self.eps_cap if self.eps is not None else (out[0].shape[0] if out else e.shape[0])
            if e.shape[0] != steps:
                raise ValueError(f"eps: every draw holds the same number of steps (the job's eps_cap, {steps}), "
                                 f"got {e.shape[0]}")
            pad = torch.zeros(e.shape[0], BATCH, Z, dtype=torch.float32)
            pad[:, :e.shape[1]] = e
            out.append(pad.to(self.device).contiguous())
        if self.eps is None:
            self.eps_cap = int(out[0].shape[0])      # (the draws' step count indexes as the job's own eps would)
        return S, keys, out

    def enable_predictive_exports(self, n_draws, seeds=None, eps=None, msq=True, z=True, rowdev=True, rowz2=True):
        """Buffers of the posterior-predictive pass (JobSet.forward_draws, nm_devpass_draws): S = n_draws latent draws per row,
        folded on the device.  seeds: one generator key per draw (default: draw_seeds(job.seed, S)); eps: a list of S tensors
        in the layout set_eps takes, used in the place of the generator.  Afterwards pred_mean[m], pred_var[m], pred_msq[m],
        pred_z[m] ([rows_alloc, D] views) and pred_rowdev[m], pred_rowz2[m] ([rows_alloc]) hold the exports of modality m,
        None where the kind was not asked for.  With z or rowz2 the observation variance exp(logvar_out) of the current
        parameters travels along (refreshed by forward_draws whenever the parameters have changed).  Refused (ValueError):
        n_draws outside 1..64, seeds / eps of another length, both given, eps draws of differing step counts."""
        S, self.pred_seeds, self.pred_eps = self._draw_request(n_draws, seeds, eps, _lib.NM_MAX_DRAWS)
        ra, M = self.tables[0].rows_alloc, len(self.kmods)
        pitch = [self.tables[m].x_pitch for m, _, _ in self.kmods]
        width = [self.tables[m].D for m, _, _ in self.kmods]
        mat = lambda on: [torch.zeros(ra, pitch[m], device=self.device)[:, :width[m]] if on else None for m in range(M)]
        row = lambda on: [torch.zeros(ra, device=self.device) if on else None for _ in range(M)]
        self.n_draws = S
        self.pred_mean, self.pred_var, self.pred_msq, self.pred_z = mat(True), mat(True), mat(msq), mat(z)
        self.pred_rowdev, self.pred_rowz2 = row(rowdev), row(rowz2)
        self.noise_var = [torch.ones(pitch[m], device=self.device) if (z or rowz2) else None for m in range(M)]
        self._nv_state = None
        self._version += 1

    def refresh_noise_var(self):
        """noise_var[m] = exp(logvar_out of decoder m) of the CURRENT parameters (in place: the table on the device keeps its
        pointers); done again only after an optimizer step or a host-side write of the parameters."""
        if getattr(self, "noise_var", None) is None or all(v is None for v in self.noise_var):
            return
        state = (self.t, self._params_epoch)
        if self._nv_state == state:
            return
        for k, (m, _, dp) in enumerate(self.kmods):
            if self.noise_var[k] is not None:
                lv = self.layout.get(self.params, f"{dp}logvar_out").reshape(-1)
                self.noise_var[k][: lv.numel()] = torch.exp(lv)
        self._nv_state = state

    def pred_structs(self):
        """This job's rows of nm_devpass_draws' two tables: ([NmDraw] * n_draws, NmPred)."""
        if getattr(self, "n_draws", None) is None:
            raise ValueError("enable_predictive_exports() first")
        draws = []
        for s in range(self.n_draws):
            d = _lib.NmDraw()
            d.seed = self.pred_seeds[s]
            d.eps = self.pred_eps[s].data_ptr() if self.pred_eps is not None else None
            draws.append(d)
        p = _lib.NmPred()
        for m in range(len(self.kmods)):
            for field in ("pred_mean", "pred_var", "pred_msq", "pred_z", "pred_rowdev", "pred_rowz2", "noise_var"):
                buf = getattr(self, field)[m]
                getattr(p, field)[m] = buf.data_ptr() if buf is not None else None
            if p.pred_z[m] and not p.noise_var[m]:
                raise ValueError("pred_z needs noise_var: the score is scaled by exp(logvar_out) + the draw variance")
        return draws, p

    def enable_likelihood_exports(self, n_draws, seeds=None, eps=None, decoders=None, per_modality=False):
        """Buffers of the likelihood pass (JobSet.forward_loglik, nm_devpass_iw): S = n_draws latent draws per row from the
        model's own posterior, their importance weights folded on the device.  seeds / eps as in enable_predictive_exports;
        decoders: the indices of the decoders whose likelihood enters the weight (default: all).  Afterwards iw_row
        [rows_alloc, 8] holds metrics.LOGLIK_ROW_COLUMNS per subject and, with per_modality, iw_recon_ll[m] [rows_alloc] the
        mean reconstruction log-likelihood of decoder m (None for a decoder left out).  Refused (ValueError): n_draws
        outside 1..1024, seeds / eps of another length, both given, an empty or out-of-range decoder list."""
        M = len(self.kmods)
        dec = list(range(M)) if decoders is None else sorted({int(m) for m in decoders})
        if not dec or dec[0] < 0 or dec[-1] >= M:
            raise ValueError(f"decoders: a non-empty subset of 0..{M - 1}, got {decoders}")
        S, keys, draws = self._draw_request(n_draws, seeds, eps, _lib.NM_MAX_IW_DRAWS)
        ra = self.tables[0].rows_alloc
        self.iw_draws, self.iw_seeds, self.iw_eps = S, keys, draws
        self.iw_mask = sum(1 << m for m in dec)
        self.iw_row = torch.zeros(ra, _lib.NM_IW_ROW_COLUMNS, device=self.device)
        self.iw_recon_ll = [torch.zeros(ra, device=self.device) if (per_modality and m in dec) else None for m in range(M)]
        self.iw_noise_var = [torch.ones(self.tables[k].x_pitch, device=self.device) if j in dec else None
                             for j, (k, _, _) in enumerate(self.kmods)]
        self.iw_ll_const = [0.0] * M
        self._iw_state = None
        self._version += 1

    def refresh_likelihood_constants(self) -> bool:
        """iw_noise_var[m] = exp(logvar_out) (in place) and iw_ll_const[m] = -0.5 sum_d (logvar_out_d + log 2 pi) (fp64, rounded
        once where the request is packed) of the CURRENT parameters; True when they changed."""
        state = (self.t, self._params_epoch)
        if self._iw_state == state:
            return False
        for k, (m, _, dp) in enumerate(self.kmods):
            if self.iw_noise_var[k] is not None:
                lv = self.layout.get(self.params, f"{dp}logvar_out").reshape(-1)
                self.iw_noise_var[k][: lv.numel()] = torch.exp(lv)
                self.iw_ll_const[k] = float(-0.5 * (lv.double() + math.log(2.0 * math.pi)).sum())
        self._iw_state = state
        return True

    def iw_structs(self):
        """This job's rows of nm_devpass_iw's two tables: ([NmDraw] * n_draws, NmIw)."""
        if getattr(self, "iw_draws", None) is None:
            raise ValueError("enable_likelihood_exports() first")
        draws = []
        for s in range(self.iw_draws):
            d = _lib.NmDraw()
            d.seed = self.iw_seeds[s]
            d.eps = self.iw_eps[s].data_ptr() if self.iw_eps is not None else None
            draws.append(d)
        q = _lib.NmIw()
        q.row, q.dec_mask = self.iw_row.data_ptr(), self.iw_mask
        for m in range(len(self.kmods)):
            q.recon_ll[m] = self.iw_recon_ll[m].data_ptr() if self.iw_recon_ll[m] is not None else None
            q.noise_var[m] = self.iw_noise_var[m].data_ptr() if self.iw_noise_var[m] is not None else None
            q.ll_const[m] = self.iw_ll_const[m]
        return draws, q

    # -- the end-to-end model's evaluation pass (nm_e2e_pass) --------------------------------------
    def _e2e_answers(self):
        """(nm_e2e_pass_ok, nm_e2e_alpha_ok) of this job's shape descriptor: the library's answers, no copy of its rules here.
        Asked again whenever the descriptor or one of the attributes it carries beside the shape has changed."""
        key = (getattr(self, "_version", 0), self.combine, getattr(self, "single_bypass", None), self.tc_weight, self.var_floor)
        hit = getattr(self, "_e2e_cache", None)
        if hit is None or hit[0] != key:
            lib, d = _lib.load(), self._shape_struct()
            hit = self._e2e_cache = (key, int(lib.nm_e2e_pass_ok(C.byref(d))), int(lib.nm_e2e_alpha_ok(C.byref(d))))
        return hit[1], hit[2]

    def e2e_ok(self) -> bool:
        """nm_e2e_pass_ok, asked of this job's shape descriptor: can the job's evaluation run on nm_e2e_pass?"""
        return self._e2e_answers()[0] == 0

    def _e2e_require_alpha(self, caller: str):
        """ValueError where the library says no route can fuse this job (nm_e2e_alpha_ok: gPoE without alpha offsets)."""
        st = self._e2e_answers()[1]
        if st != 0:
            raise ValueError(f"{caller}: nm_e2e_alpha_ok refuses the job with status {st} ({_lib.load().nm_status_string(st).decode()}): "
                             f"gPoE weighs the experts by softmax(alpha) and this model registers no alpha parameters")

    def enable_endtoend_exports(self, rows=True, loc=False, sqerr=False, rowdev=True, latent=True, decoders=None):
        """Buffers of the end-to-end model's evaluation (JobSet.forward_endtoend, nm_e2e_pass): out_logits always; with
        rows, e2e_row [rows_alloc, 8] = metrics.ENDTOEND_ROW_COLUMNS per subject; out_loc / out_sqerr / out_rowdev of every
        decoder (both banks: health k < M, disease M <= k < 2 M) as asked; decoders: the indices whose loc / sqerr /
        rowdev exports the compact pass writes (default: all; the row table does not depend on it).  latent: out_mu /
        out_logvar / out_z are results the caller reads; the buffers are allocated either way -- the descriptor's classifier
        reads out_mu / out_z (nm_validate_job) and the two-launch route reads all three."""
        if self.spec.kind != "endtoend" or not self.spec.classifier_layers:
            raise ValueError("enable_endtoend_exports: an end-to-end model (kind 'endtoend' with a classifier) is needed")
        self._e2e_require_alpha("enable_endtoend_exports")
        nk = len(self.kmods)
        dec = list(range(nk)) if decoders is None else sorted({int(m) for m in decoders})
        if dec and (dec[0] < 0 or dec[-1] >= nk):
            raise ValueError(f"decoders: a subset of 0..{nk - 1}, got {decoders}")
        self.enable_exports(loc=loc, sqerr=sqerr, rowdev=rowdev, latent=True)
        if self.out_logits is None:
            self.out_logits = torch.zeros(self.tables[0].rows_alloc, _lib.NM_MAX_CLASSES, device=self.device)
        self.e2e_latent = bool(latent)
        self.e2e_mask = sum(1 << m for m in dec)
        self.e2e_row = torch.zeros(self.tables[0].rows_alloc, _lib.NM_E2E_ROW_COLUMNS, device=self.device) if rows else None
        self.e2e_enabled = True
        self._version += 1

    def e2e_struct(self, use_mean: bool) -> "_lib.NmE2e":
        if not getattr(self, "e2e_enabled", False):
            raise ValueError("enable_endtoend_exports() first")
        q = _lib.NmE2e()
        q.row = self.e2e_row.data_ptr() if self.e2e_row is not None else None
        q.use_mean, q.want_mask = int(bool(use_mean)), self.e2e_mask
        return q

    # -- the regression model's evaluation pass (nm_fi_pass) ----------------------------------------
    def fi_ok(self) -> bool:
        """nm_fi_pass_ok, asked of this job's shape descriptor: can the job's FI evaluation run on nm_fi_pass?  Asked again
        whenever the descriptor or one of the attributes it carries beside the shape has changed."""
        key = (getattr(self, "_version", 0), self.combine, getattr(self, "single_bypass", None), self.tc_weight, self.var_floor)
        hit = getattr(self, "_fi_cache", None)
        if hit is None or hit[0] != key:
            hit = self._fi_cache = (key, int(_lib.load().nm_fi_pass_ok(C.byref(self._shape_struct()))))
        return hit[1] == 0

    def enable_fi_exports(self, rows=True, draws=False, loc=False, sqerr=False, rowdev=True, latent=True, decoders=None):
        """Buffers of the regression model's evaluation (JobSet.forward_fi, nm_fi_pass): out_fi_pred always; with rows,
        fi_row [rows_alloc, 8] = metrics.FI_ROW_COLUMNS per subject; with draws, fi_draws [rows_alloc, n_draws] (allocated by
        forward_fi for the number of draws it is asked for); out_loc / out_sqerr / out_rowdev of every decoder and the latent
        exports as asked (they hold draw 0); decoders: the indices whose loc / sqerr / rowdev exports are written
        (default: all; the row table does not depend on it)."""
        if self.spec.kind != "regression":
            raise ValueError("enable_fi_exports: a regression model (kind 'regression') is needed")
        nk = len(self.kmods)
        dec = list(range(nk)) if decoders is None else sorted({int(m) for m in decoders})
        if dec and (dec[0] < 0 or dec[-1] >= nk):
            raise ValueError(f"decoders: a subset of 0..{nk - 1}, got {decoders}")
        self.enable_exports(loc=loc, sqerr=sqerr, rowdev=rowdev, latent=latent)
        if not latent:
            self.out_mu = self.out_logvar = self.out_z = None
        self.fi_mask = sum(1 << m for m in dec)
        self.fi_row = torch.zeros(self.tables[0].rows_alloc, _lib.NM_FI_ROW_COLUMNS, device=self.device) if rows else None
        self.fi_want_draws, self.fi_draws = bool(draws), None
        self.fi_enabled = True
        self._version += 1

    def fi_struct(self, use_mean: bool, n_draws: int) -> "_lib.NmFi":
        if not getattr(self, "fi_enabled", False):
            raise ValueError("enable_fi_exports() first")
        if self.fi_want_draws and (self.fi_draws is None or self.fi_draws.shape[1] != n_draws):
            self.fi_draws = torch.zeros(self.tables[0].rows_alloc, n_draws, device=self.device)
        q = _lib.NmFi()
        q.row = self.fi_row.data_ptr() if self.fi_row is not None else None
        q.fi_draws = self.fi_draws.data_ptr() if self.fi_want_draws else None
        q.use_mean, q.want_mask = int(bool(use_mean)), self.fi_mask
        return q

    def set_latent_exports(self, on: bool):
        """Switch the joint-latent exports (out_mu / out_logvar / out_z) of a job that has them off and back on; the
        buffers are kept.  Off, a reconstruction-only forward (JobSet.forward(loss=False)) can run on the compact kernels."""
        if on == (self.out_mu is not None):
            return
        if on:
            stash = getattr(self, "_latent_stash", None)
            if stash is None:
                ra, Z = self.tables[0].rows_alloc, self.spec.latent
                stash = tuple(torch.zeros(ra, Z, device=self.device) for _ in range(3))
            self.out_mu, self.out_logvar, self.out_z = stash
        else:
            self._latent_stash = (self.out_mu, self.out_logvar, self.out_z)
            self.out_mu = self.out_logvar = self.out_z = None
        self._version += 1

    # -- the decoder pass (nm_decode_pass) -------------------------------------------------------
    def decode_ok(self) -> bool:
        """nm_decode_pass_ok for this job: exactly what latent_ok() admits -- the encoder half and the decoder half cover the
        same models (tests/test_cabi_decode_cpu.py holds this to the library)."""
        return self.latent_ok()

    def enable_decode_exports(self, n_rows, n_cells=0, loc=True, sqerr=False, rowdev=False, decoders=None):
        """Buffers of the decoder pass (JobSet.decode, nm_decode_pass) for a request of n_rows latent rows -- its own row count,
        not the tables' -- decoded under the rows' own covariates (n_cells = 0) or under each of n_cells rows of a covariate
        grid (1..64).  decoders: the modalities to decode (None: every one); a decoder left out is skipped by the kernel.
        Afterwards dec_loc[m], dec_sqerr[m] ([cells, n_rows, D] views, cells = max(n_cells, 1)) and dec_rowdev[m] ([cells,
        n_rows]) hold the exports of decoder m, None where the decoder or the kind was not asked for; dec_full["loc" /
        "sqerr" / "rowdev"][m] are the whole buffers ([cells, rows_alloc, x_pitch] / [cells, rows_alloc]).  sqerr / rowdev
        are taken against x (set_decode_inputs).  Refused (ValueError): n_cells outside 0..64, no rows, loc=False (the
        kernel skips a decoder without loc), a decoder index beyond the model's."""
        R, G, M = int(n_rows), int(n_cells), len(self.kmods)
        if not 0 <= G <= _lib.NM_MAX_CELLS:
            raise ValueError(f"n_cells must be 0 to {_lib.NM_MAX_CELLS}, got {n_cells}")
        if R < 1:
            raise ValueError(f"n_rows must be at least 1, got {n_rows}")
        if not loc:
            raise ValueError("loc=False: the kernel skips a decoder without loc -- leave it out of `decoders` instead")
        decoders = tuple(range(M)) if decoders is None else tuple(int(m) for m in decoders)
        if not decoders or any(m < 0 or m >= M or m >= _lib.NM_MAX_EXP for m in decoders):
            raise ValueError(f"decoders: modalities 0..{min(M, _lib.NM_MAX_EXP) - 1}, at least one")
        ra, cells = (R + BATCH - 1) // BATCH * BATCH, max(G, 1)
        pitch = [self.tables[m].x_pitch for m, _, _ in self.kmods]
        width = [self.tables[m].D for m, _, _ in self.kmods]
        mat = lambda on: [torch.zeros(cells, ra, pitch[m], device=self.device) if on and m in decoders else None for m in range(M)]
        row = lambda on: [torch.zeros(cells, ra, device=self.device) if on and m in decoders else None for m in range(M)]
        self.dec_rows, self.dec_rows_alloc, self.dec_cells, self.dec_decoders = R, ra, G, decoders
        self.dec_full = {"loc": mat(True), "sqerr": mat(sqerr), "rowdev": row(rowdev)}
        cut = lambda ts: [t[:, :R, :width[m]] if t is not None else None for m, t in enumerate(ts)]
        self.dec_loc, self.dec_sqerr = cut(self.dec_full["loc"]), cut(self.dec_full["sqerr"])
        self.dec_rowdev = [t[:, :R] if t is not None else None for t in self.dec_full["rowdev"]]
        self.dec_z = self.dec_cgrid = None
        self.dec_cz, self.dec_x = [None] * M, [None] * M
        self._dec_epoch += 1

    def set_decode_inputs(self, z, c=None, c_grid=None, x="tables"):
        """Inputs of the decoder pass.  z: [n_rows, Z] fp32 latent rows (copied).  Per-row requests (n_cells = 0): c is one
        covariate table [n_rows, C] for every decoder, a list with one per decoder, or None -- the job's own tables' packed
        covariates, and then n_rows must equal the tables' rows.  Grid requests: c_grid [n_cells, C], one row per cell.
        Covariates are packed to bf16 c | 1 | 0 rows of pitch Cz (pack_covariates: the bytes Table holds in .cz for the same
        c).  x: "tables" -- sqerr / rowdev are taken against the tables' own x (n_rows must equal the tables' rows) -- or
        None (requests with loc alone; the default falls back to None where neither sqerr nor rowdev was asked for)."""
        if self.dec_rows is None:
            raise ValueError("enable_decode_exports() first")
        R, ra, G, M, Z = self.dec_rows, self.dec_rows_alloc, self.dec_cells, len(self.kmods), self.spec.latent
        z = torch.as_tensor(np.asarray(z) if not torch.is_tensor(z) else z)
        if z.dim() != 2 or int(z.shape[0]) != R or int(z.shape[1]) != Z:
            raise ValueError(f"z must be [{R}, {Z}], got {tuple(z.shape)}")
        if self.dec_z is None:
            self.dec_z = torch.zeros(ra, Z, device=self.device)
        self.dec_z[:R].copy_(z.to(device=self.device, dtype=torch.float32))
        Cz, N = self.tables[0].Cz, self.tables[0].N
        if G > 0:
            if c is not None or c_grid is None:
                raise ValueError("a grid request takes c_grid (one covariate row per cell), not per-row c")
            g = torch.as_tensor(np.asarray(c_grid) if not torch.is_tensor(c_grid) else c_grid)
            if g.dim() != 2 or int(g.shape[0]) != G or int(g.shape[1]) != self.spec.net_c_dim:
                raise ValueError(f"c_grid must be [{G}, {self.spec.net_c_dim}], got {tuple(g.shape)}")
            self.dec_cgrid = pack_covariates(g, Cz, G, self.device)
            self.dec_cz = [None] * M
        else:
            if c_grid is not None:
                raise ValueError("c_grid needs a grid request: enable_decode_exports(n_rows, n_cells=G)")
            if c is None:
                if R != N or ra != self.tables[0].rows_alloc:
                    raise ValueError(f"c=None reads the tables' own covariates: the request has {R} rows, the tables {N}")
                self.dec_cz = [self.tables[m].cz for m, _, _ in self.kmods]
            else:
                per = list(c) if isinstance(c, (list, tuple)) else [c] * M
                if len(per) != M:
                    raise ValueError(f"c: one covariate table, or one per decoder ({M}), got {len(per)}")
                packed = {}
                for t in per:
                    if int(t.shape[0]) != R or int(t.shape[1]) != self.spec.net_c_dim:
                        raise ValueError(f"c must be [{R}, {self.spec.net_c_dim}], got {tuple(t.shape)}")
                    if id(t) not in packed:
                        packed[id(t)] = pack_covariates(t, Cz, ra, self.device)
                self.dec_cz = [packed[id(t)] for t in per]
            self.dec_cgrid = None
        wants_x = any(t is not None for t in self.dec_full["sqerr"]) or any(t is not None for t in self.dec_full["rowdev"])
        if x is None or (isinstance(x, str) and x == "tables" and not wants_x):
            if wants_x:
                raise ValueError("sqerr / rowdev are taken against x: x=None leaves them without it")
            self.dec_x = [None] * M
        elif isinstance(x, str) and x == "tables":
            if R != N or ra != self.tables[0].rows_alloc:
                raise ValueError(f'x="tables" reads the tables\' own x: the request has {R} rows, the tables {N}')
            self.dec_x = [self.tables[m].x_f32 for m, _, _ in self.kmods]
        else:
            raise ValueError('x: "tables" or None')
        self._dec_epoch += 1

    def decode_struct(self) -> "_lib.NmDecode":
        """This job's entry of nm_decode_pass' request table, validated (check_decode_request) before it travels."""
        if self.dec_rows is None or self.dec_z is None:
            raise ValueError("enable_decode_exports() and set_decode_inputs() first")
        M = len(self.kmods)
        full = self.dec_full
        check_decode_request(self.dec_rows, self.dec_rows_alloc, self.dec_cells, self.spec.latent, self.tables[0].Cz,
                             [self.tables[m].x_pitch for m, _, _ in self.kmods], self.dec_z, self.dec_cgrid, self.dec_cz,
                             self.dec_x, full["loc"], full["sqerr"], full["rowdev"])
        r = _lib.NmDecode()
        r.z, r.n_rows, r.rows_alloc, r.n_cells = self.dec_z.data_ptr(), self.dec_rows, self.dec_rows_alloc, self.dec_cells
        r.cgrid = self.dec_cgrid.data_ptr() if self.dec_cgrid is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        for m in range(M):
            r.cz[m], r.x[m] = ptr(self.dec_cz[m]), ptr(self.dec_x[m])
            r.loc[m], r.sqerr[m], r.rowdev[m] = ptr(full["loc"][m]), ptr(full["sqerr"][m]), ptr(full["rowdev"][m])
        return r

    # -- the chart pass (nm_chart_pass) ----------------------------------------------------------
    def chart_ok(self) -> bool:
        """nm_chart_pass_ok for this job: exactly decode_ok() (tests/test_cabi_chart_cpu.py holds this to the library)."""
        return self.decode_ok()

    def enable_chart_exports(self, n_rows, n_cells, decoders=None, loc=False, chart=True):
        """Buffers of the chart pass (JobSet.chart, nm_chart_pass) for a request of n_rows latent rows decoded under each of
        n_cells rows of a covariate grid (1..64), the per-cell moments folded in the kernel.  decoders: the modalities wanted
        (None: every one); a decoder left out is skipped.  Afterwards chart[m] ([n_cells, D, 4] fp64 view: CHART_COLUMNS of
        metrics) holds the table of decoder m, chart_full["part" / "chart" / "loc"][m] the whole buffers; loc=True adds
        the [n_cells, rows_alloc, x_pitch] export of nm_decode_pass (chart_loc[m]: [n_cells, n_rows, D] views); chart=False
        with loc=True asks for loc alone (the cell-parallel decode).  Refused (ValueError): n_cells outside 1..64, n_rows
        outside 1..NM_CHART_MAX_ROWS, a decoder index beyond the model's, neither chart nor loc."""
        R, G, M = int(n_rows), int(n_cells), len(self.kmods)
        if not 1 <= G <= _lib.NM_MAX_CELLS:
            raise ValueError(f"n_cells must be 1 to {_lib.NM_MAX_CELLS}, got {n_cells}")
        if not 1 <= R <= _lib.NM_CHART_MAX_ROWS:
            raise ValueError(f"n_rows must be 1 to {_lib.NM_CHART_MAX_ROWS}, got {n_rows}")
        if not chart and not loc:
            raise ValueError("chart=False and loc=False: nothing is wanted")
        decoders = tuple(range(M)) if decoders is None else tuple(int(m) for m in decoders)
        if not decoders or any(m < 0 or m >= M or m >= _lib.NM_MAX_EXP for m in decoders):
            raise ValueError(f"decoders: modalities 0..{min(M, _lib.NM_MAX_EXP) - 1}, at least one")
        ra = (R + BATCH - 1) // BATCH * BATCH
        pitch = [self.tables[m].x_pitch for m, _, _ in self.kmods]
        width = [self.tables[m].D for m, _, _ in self.kmods]
        f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=self.device)
        per = lambda on, make: [make(m) if on and m in decoders else None for m in range(M)]
        self.chart_rows, self.chart_rows_alloc, self.chart_cells, self.chart_decoders = R, ra, G, decoders
        self.chart_full = {"part": per(chart, lambda m: f64(G, ra // 128, pitch[m], 2)),
                           "chart": per(chart, lambda m: f64(G, pitch[m], _lib.NM_CHART_COLUMNS)),
                           "loc": per(loc, lambda m: torch.zeros(G, ra, pitch[m], device=self.device))}
        self.chart = [t[:, :width[m]] if t is not None else None for m, t in enumerate(self.chart_full["chart"])]
        self.chart_loc = [t[:, :R, :width[m]] if t is not None else None for m, t in enumerate(self.chart_full["loc"])]
        self.chart_z = self.chart_cgrid = None
        self._chart_epoch += 1

    def set_chart_inputs(self, z, c_grid):
        """Inputs of the chart pass: z [n_rows, Z] fp32 latent rows (copied) and c_grid [n_cells, C], one covariate row per
        cell, packed to bf16 c | 1 | 0 rows (pack_covariates), as set_decode_inputs does for a grid request."""
        if self.chart_rows is None:
            raise ValueError("enable_chart_exports() first")
        R, ra, G, Z = self.chart_rows, self.chart_rows_alloc, self.chart_cells, self.spec.latent
        z = torch.as_tensor(np.asarray(z) if not torch.is_tensor(z) else z)
        if z.dim() != 2 or int(z.shape[0]) != R or int(z.shape[1]) != Z:
            raise ValueError(f"z must be [{R}, {Z}], got {tuple(z.shape)}")
        if self.chart_z is None:
            self.chart_z = torch.zeros(ra, Z, device=self.device)
        self.chart_z[:R].copy_(z.to(device=self.device, dtype=torch.float32))
        g = torch.as_tensor(np.asarray(c_grid) if not torch.is_tensor(c_grid) else c_grid)
        if g.dim() != 2 or int(g.shape[0]) != G or int(g.shape[1]) != self.spec.net_c_dim:
            raise ValueError(f"c_grid must be [{G}, {self.spec.net_c_dim}], got {tuple(g.shape)}")
        self.chart_cgrid = pack_covariates(g, self.tables[0].Cz, G, self.device)
        self._chart_epoch += 1

    def chart_struct(self) -> "_lib.NmChart":
        """This job's entry of nm_chart_pass' request table, validated (check_chart_request) before it travels."""
        if self.chart_rows is None or self.chart_z is None:
            raise ValueError("enable_chart_exports() and set_chart_inputs() first")
        full = self.chart_full
        check_chart_request(self.chart_rows, self.chart_rows_alloc, self.chart_cells, self.spec.latent, self.tables[0].Cz,
                            [self.tables[m].x_pitch for m, _, _ in self.kmods], self.chart_z, self.chart_cgrid,
                            full["part"], full["chart"], full["loc"])
        r = _lib.NmChart()
        r.z, r.n_rows, r.rows_alloc, r.n_cells = self.chart_z.data_ptr(), self.chart_rows, self.chart_rows_alloc, self.chart_cells
        r.cgrid = self.chart_cgrid.data_ptr()
        ptr = lambda t: t.data_ptr() if t is not None else None
        for m in range(len(self.kmods)):
            r.part[m], r.chart[m], r.loc[m] = ptr(full["part"][m]), ptr(full["chart"][m]), ptr(full["loc"][m])
        return r

    # -- descriptor ----------------------------------------------------------------------------
    def kernel_combine(self) -> str:
        """The combiner the descriptor carries.  gPoE weighs the experts by softmax(alpha); a one-expert model whose class
        has no alpha parameter (class cVAE: its descriptor holds alpha = -1) with the bypass off would make every kernel read
        the float in front of the parameter buffer for it -- an address that need not be mapped.  One expert's softmax weight
        is exactly 1 whatever alpha holds, and 1 * (1 / var) is 1 / var: such a job is a product of experts, bit for bit,
        and is described as one."""
        if self.combine == "gpoe" and self.spec.M == 1 and "alpha_m_list.0" not in self.layout.offsets:
            return "poe"
        return self.combine

    def _shape_struct(self) -> _lib.NmJob:
        """A descriptor holding the model's shape alone -- decoders, experts, widths, latent, output kind, the head's blocks
        and offsets -- and no buffer: what struct() starts from, and what the library's *_ok predicates are asked about
        where no device is needed (e2e_ok)."""
        s, j = self.spec, _lib.NmJob()
        j.M, j.M_enc, j.C, j.L, j.Z = len(self.kmods), s.M, s.net_c_dim, len(s.hidden), s.latent
        # DMVAE family: ReLU, sigmoid / squared-error output, private latent columns, learnable loss weights
        j.act_slope = 0.0 if s.is_dm else 0.01
        j.out_kind = 1 if s.is_dm else 0
        j.n_private = s.n_private
        j.w_off = self.layout.offsets["weights"] if s.kind == "weighted_dmvae" else -1
        j.var_floor, j.tc_weight = self.var_floor, self.tc_weight
        for i, h in enumerate(s.hidden):
            j.H[i] = h
        j.wide = int(s.wide)
        j.combine = _lib.NM_COMBINE[self.kernel_combine()]
        j.single_bypass = 1 if self.single_bypass else 0
        for k in range(len(self.kmods)):              # every tensor's offset (alpha: -1 where the class registers none)
            self.layout.fill_modality(j.mod[k], k)
        self.layout.fill_head(j)
        return j

    def struct(self) -> _lib.NmJob:
        s, j = self.spec, self._shape_struct()
        j.n_rows = self.tables[0].N
        j.non_linear = 1 if (s.non_linear or s.is_dm) else 0        # (torch.relu unconditionally, cVAE.py:1462-1463)
        j.dephase = int(self.dephase_sleeps)
        k0 = self.tables[0].c_key
        j.shared_cov = 1 if (k0 is not None and all(t.c_key == k0 for t in self.tables)) else 0
        self._shared_cov = int(j.shared_cov)
        j.loss_cap, j.eps_cap = self.loss_cap, self.eps_cap
        j.lr, j.beta1, j.beta2, j.adam_eps = self.lr, self.betas[0], self.betas[1], self.adam_eps
        j.adam_off = self.t - self.step
        j.lr_table = self.lr_table.data_ptr() if self.lr_table is not None else None
        j.lr_cap = int(self.lr_table.numel()) if self.lr_table is not None else 0
        j.kl_weight, j.ll_weight = self.kl_weight, self.ll_weight
        j.params, j.adam_m, j.adam_v = self.params.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr()
        j.grads = self.grads.data_ptr()
        j.eps = self.eps.data_ptr() if self.eps is not None else None
        j.seed = self.seed
        j.loss_log = self.loss_log.data_ptr()
        j.workspace = self._ws.data_ptr()
        j.workspace_stride = self.ws_bytes
        j.n_params = int(self.params.numel())
        j.gpart = self._gpart.data_ptr() if self._gpart is not None else None
        j.gpart_stride = self.gpart_stride
        j.wsh = self._wsh.data_ptr()
        j.out_mu = self.out_mu.data_ptr() if self.out_mu is not None else None
        j.out_logvar = self.out_logvar.data_ptr() if self.out_logvar is not None else None
        j.out_z = self.out_z.data_ptr() if self.out_z is not None else None
        j.dz_extra = self.dz_extra.data_ptr() if self.dz_extra is not None else None
        if j.reg_head:
            self.prepare_regression()
            j.reg_resid, j.reg_dres = self.reg_resid.data_ptr(), self.reg_dres.data_ptr()
        j.reg_lambda = self.reg_lambda
        j.fi_target = self.fi_target.data_ptr() if self.fi_target is not None else None
        j.out_fi_pred = self.out_fi_pred.data_ptr() if self.out_fi_pred is not None else None
        if j.cls_classes and (self.out_z is None or self.out_mu is None):
            j.cls_layers, j.cls_classes = 0, 0        # the head reads the exported latent
        j.cls_train, j.cls_use_mu = int(self.cls_train), int(self.cls_use_mu)
        j.cls_dropout, j.cls_margin = self.cls_dropout, self.cls_margin
        j.cls_w_ce, j.cls_w_contrast = self.cls_w_ce, self.cls_w_contrast
        j.labels = self.labels.data_ptr() if self.labels is not None else None
        j.out_logits = self.out_logits.data_ptr() if self.out_logits is not None else None
        j.dz_out = self.dz_extra.data_ptr() if self.dz_extra is not None else None
        for k, (m, _, _) in enumerate(self.kmods):
            t = self.tables[m]
            md = j.mod[k]
            md.D, md.Kx, md.x_pitch, md.Cz = t.D, t.Kx, t.x_pitch, t.Cz
            md.x_f32, md.xb, md.cz = t.x_f32.data_ptr(), t.xb.data_ptr(), t.cz.data_ptr()
            self.layout.fill_modality(md, k)
            md.out_loc = self.out_loc[k].data_ptr() if self.out_loc[k] is not None else None
            md.out_sqerr = self.out_sqerr[k].data_ptr() if self.out_sqerr[k] is not None else None
            md.out_rowdev = self.out_rowdev[k].data_ptr() if self.out_rowdev[k] is not None else None
            md.dloc_extra = self.dloc_extra[k].data_ptr() if self.dloc_extra[k] is not None else None
            md.dloc_rowcoef = self.dloc_rowcoef[k].data_ptr() if self.dloc_rowcoef[k] is not None else None
            j.rowcoef_out[k] = md.dloc_rowcoef
        if not s.wide or s.kind == "regression":
            nb = int(_lib.load().nm_fill_shadow(C.byref(j)))       # shadow-image offsets of every modality
            if nb != self._wsh.numel():
                raise _lib.NmError(f"shadow size changed: {nb} vs {self._wsh.numel()} bytes")
        _lib.check(_lib.load().nm_validate_job(C.byref(j)), "nm_validate_job")
        return j

    # -- state_dict interchange (reference key names) --------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach().cpu().clone() for k, v in self.layout.unflatten(self.params).items()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]):
        self.params.copy_(self.layout.flatten(state, device=self.device))
        self.shadow_dirty = True
        self._params_epoch += 1

    def params_changed(self):
        """Call after writing ``params`` from the host side (an external optimizer, a hand edit): the bf16 shadow
        images the kernels read are rebuilt before the next launch."""
        self.shadow_dirty = True
        self._params_epoch += 1

    def grads_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach().cpu().clone() for k, v in self.layout.unflatten(self.grads).items()}

    def adam_dicts(self):
        m = {k: v.detach().cpu().clone() for k, v in self.layout.unflatten(self.adam_m).items()}
        v = {k: v.detach().cpu().clone() for k, v in self.layout.unflatten(self.adam_v).items()}
        return m, v

    @property
    def batches_per_epoch(self) -> int:
        return math.ceil(self.tables[0].N / BATCH)


# the launches that leave hand-off error words behind (nm_split_errors), by the kind their error message names
_HANDOFF_KINDS = {"nm_launch_split": "split", "nm_launch_rowsplit": "rowsplit", "nm_launch_rowsplit_mixed": "rowsplit",
                  "nm_train_steps_head_split": "split"}


class JobSet:
    """Device array of job descriptors = the unit one launch runs (one workgroup per job)."""

    def __init__(self, jobs: Sequence[Job]):
        if not jobs:
            raise ValueError("empty job set")
        self.jobs = list(jobs)
        self.wide = bool(jobs[0].spec.wide)
        if any(bool(j.spec.wide) != self.wide for j in jobs):
            raise ValueError("a job set holds either fused-kernel shapes or general-shape (wide) models, not both")
        self.device = jobs[0].device
        self.lib = _lib.load()
        self._dev = None
        self._sig = None
        self._dephase_vals = None        # the start offsets this set last assigned (_set_dephase)
        self._split_pending = False      # a split launch has run since the hand-off error words were last read
        self._pending_kinds = set()      # ... of which kinds ("split", "rowsplit"): the error message names their switch
        self._err_kinds = set()          # the kinds behind the error words in flight
        self._err_inflight = None        # (event, pinned host copy) of the error words being fetched
        self._err_dev = self._err_host = None
        self._plain_sig = self._plain_all = None   # plain_pick(): the jobs' descriptor versions it last judged, and the verdict
        self.last_launch = None          # {"entry", "flags", "plain"} of the set's last launch (plain: the plain-training kernel)

    @functools.cached_property
    def _cus(self) -> int:
        return torch.cuda.get_device_properties(self.device).multi_processor_count

    def check_split_errors(self, block: bool = True):
        """Raise NmError if a hand-off of a split launch (one workgroup per modality) timed out: the job's workgroups left
        that launch, its parameters are not to be trusted.  The error words are fetched asynchronously (a small kernel + a
        copy into pinned memory behind the launch); block=True -- everything that reads results: assert_finite, losses,
        sweep.save_model -- waits for the words of every split launch so far; block=False -- before the next launch of
        this set -- only looks at words that have already arrived, so a loop of launches is never stalled by the check."""
        if self._err_inflight is not None:
            ev, host = self._err_inflight
            if block:
                ev.synchronize()
            if ev.query():
                self._err_inflight = None
                kinds = self._err_kinds
                vals = host.tolist()
                shape = [i for i, v in enumerate(vals) if v == _lib.NM_SYNC_ERR_SHAPE]
                plain = [i for i, v in enumerate(vals) if v == _lib.NM_SYNC_ERR_PLAIN]
                bad = [i for i, v in enumerate(vals) if v not in (0, _lib.NM_SYNC_ERR_SHAPE, _lib.NM_SYNC_ERR_PLAIN)]
                if plain:
                    raise _lib.NmError(f"plain-training launch (NM_F_PLAIN): job(s) {plain[:8]} need the generic step kernel "
                                       f"(nm_plain_ok: a head, extra gradients, exports, a model kind beyond the plain trunk) and "
                                       f"were refused by the kernel; their parameters were not updated -- run them with "
                                       f"plain=False or NMHIP_PLAIN=0")
                if shape:
                    raise _lib.NmError(f"row-split launch: job(s) {shape[:8]} exceed the Adam sweep's tables (passes, vector "
                                       f"segments or vector elements; nm_rowsplit_ok) -- or the launch's group map lists them "
                                       f"with a modality count that is not theirs -- and were refused by the kernel; their "
                                       f"parameters were not updated -- run them with rowsplit=1 or NMHIP_ROWSPLIT=0")
                if bad:
                    # (the switch that turns the pending launch kind off: row slices / one workgroup per modality)
                    switch = " / ".join(v for kd, v in (("rowsplit", "NMHIP_ROWSPLIT=0"), ("split", "NMHIP_SPLIT=0"))
                                        if kd in kinds) or "NMHIP_SPLIT=0"
                    what = "row-split" if kinds == {"rowsplit"} else "split"
                    raise _lib.NmError(f"{what} launch: the hand-off between the workgroups of job(s) {bad[:8]} timed out "
                                       f"(the parts of a model must all be resident at once: another stream or process "
                                       f"occupying CUs breaks that); their parameters are not valid -- re-run with {switch}")
        if self._split_pending and self._dev is not None and self._err_inflight is None:
            n = len(self.jobs)
            if self._err_dev is None:
                self._err_dev = torch.zeros(n, dtype=torch.int32, device=self.device)
                self._err_host = torch.zeros(n, dtype=torch.int32).pin_memory()
            _lib.check(self.lib.nm_split_errors(self._dev.data_ptr(), n, self._err_dev.data_ptr(), 1,
                                                _stream_ptr(self.device)), "nm_split_errors")
            self._err_host.copy_(self._err_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._err_inflight = (ev, self._err_host)
            self._err_kinds, self._pending_kinds = self._pending_kinds, set()
            self._split_pending = False
            if block:
                self.check_split_errors(True)

    def _set_dephase(self):
        """Start offsets of the jobs of a long launch (nm_job_t.dephase): workgroup b lands on XCD b mod 8 (observed
        placement, speed only), so the 32 jobs that share an XCD -- its L2 and its link to memory -- are spread
        evenly over one step, and the XCDs are staggered against each other by a fraction of that spacing.  Sets of
        fewer than 16 jobs start at once."""
        vals = self._dephase_vals
        # (host time of a launch matters: it precedes the launch -- so the offsets are computed once per set; a job that
        #  another set has re-timed in between is noticed by comparing the values this set assigned)
        if vals is not None and all(j.dephase_sleeps == v for j, v in zip(self.jobs, vals)):
            return
        n = len(self.jobs)
        per_xcd = max(1, (n + 7) // 8)
        for b, j in enumerate(self.jobs):
            # ~2.05 ns per parameter and step with the chip full (measured: 0.73 ms for 355 k parameters)
            step_us = j.layout.n_params * 2.05e-3
            frac = 0.0 if n < 16 else ((b >> 3) + (b & 7) / 8) / per_xcd
            s = int(round(step_us * frac))
            if s != j.dephase_sleeps:
                j.dephase_sleeps = s
                j._version += 1
        self._dephase_vals = [j.dephase_sleeps for j in self.jobs]

    def _upload(self, n_tiles: int = 1):
        """Descriptor array on the device; rebuilt only when a job's descriptor changed (the
        optimizer step count rides on adam_off = t - step, constant while both advance)."""
        self.check_split_errors(block=False)
        self._set_dephase()
        for j in self.jobs:
            j._ensure_workspace(n_tiles)
        sig = tuple((j._version, j.t - j.step) for j in self.jobs)
        if self._dev is None or sig != self._sig:
            arr = (_lib.NmJob * len(self.jobs))(*[j.struct() for j in self.jobs])
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self._dev = host.to(self.device)
            self._sig = sig
        if self.wide:                                # (no shadow images but a regression head's first layer)
            for j in self.jobs:
                j.shadow_dirty = j.shadow_dirty and j.spec.kind == "regression"
        if any(j.shadow_dirty for j in self.jobs):
            _lib.check(self.lib.nm_sync_shadow(self._dev.data_ptr(), len(self.jobs), _stream_ptr(self.device)), "nm_sync_shadow")
            for j in self.jobs:
                j.shadow_dirty = False
        return self._dev.data_ptr()

    def _issue(self, entry: str, n_tiles: int, *args):
        """Every launch of the set: the descriptors up with n_tiles workspace tiles per job, then the C entry point
        `entry`(jobs, n_jobs, *args, stream).  A split / row-split launch leaves its hand-off error words to be read."""
        ptr = self._upload(n_tiles)
        # (a ctypes array -- the per-job modality counts of nm_launch_rowsplit_mixed -- passes as it is)
        args = [a if isinstance(a, C.Array) else int(a) for a in args]
        _lib.check(getattr(self.lib, entry)(ptr, len(self.jobs), *args, _stream_ptr(self.device)), entry)
        kind = _HANDOFF_KINDS.get(entry)
        if kind is not None:
            self._split_pending = True
            self._pending_kinds.add(kind)

    def plain_pick(self) -> bool:
        """Does every job of the set pass Job.plain_ok (the plain-training kernel serves the set's whole-batch training
        launches)?  Judged once per state of the jobs' descriptors; NMHIP_PLAIN=0 switches the kernel off."""
        if self.wide or os.environ.get("NMHIP_PLAIN", "1") == "0":
            return False
        sig = tuple(j._version for j in self.jobs)
        if sig != self._plain_sig:
            self._plain_sig, self._plain_all = sig, all(j.plain_ok() for j in self.jobs)
        return self._plain_all

    def _launch(self, step0, steps_per_tile, n_tiles, flags, scalar_tr=False, plain: Optional[bool] = None):
        """nm_launch (general-shape sets: nm_launch_wide).  A training launch -- backward + Adam, nothing else but the
        diagnostic flags -- of a set that passes plain_pick() carries NM_F_PLAIN: the step kernel's plain-training
        instantiation, bit-identical results.  plain=False keeps the generic kernel; plain=True insists (ValueError if the
        launch or a job does not qualify)."""
        entry = "nm_launch_wide" if self.wide else ("nm_launch_scalar_tr" if scalar_tr else "nm_launch")
        mode = flags & (_lib.NM_F_BACKWARD | _lib.NM_F_ADAM | _lib.NM_F_GRADS | _lib.NM_F_EXPORT | _lib.NM_F_ZGIVEN)
        use_plain = (plain is not False and entry == "nm_launch" and n_tiles == 1
                     and mode == (_lib.NM_F_BACKWARD | _lib.NM_F_ADAM) and self.plain_pick())
        if plain and not use_plain:
            raise ValueError("plain=True: the plain-training kernel serves whole-batch training launches of sets whose jobs all "
                             "pass Job.plain_ok() (and NMHIP_PLAIN is not 0)")
        if use_plain:
            flags |= _lib.NM_F_PLAIN
        self._issue(entry, n_tiles, step0, steps_per_tile, n_tiles, flags)
        self.last_launch = {"entry": entry, "flags": int(flags), "plain": bool(use_plain)}
        if use_plain:                                # (the kernel's own guard reports through the jobs' error words)
            self._split_pending = True
            self._pending_kinds.add("plain")

    def _launch_split(self, step0, n_steps, flags):
        """nm_launch_split: every model as one workgroup per modality (small sets; see split_parts)."""
        self._issue("nm_launch_split", 1, len(self.jobs[0].kmods), step0, n_steps, flags)

    def split_parts(self) -> int:
        """Workgroups per model for a training launch: the M modalities of a model as separate workgroups when the
        set is small enough for all of them to be resident at once (nm_launch_split), else 1.  NMHIP_SPLIT=0 / 1
        forces one / insists on several."""
        M = len(self.jobs[0].kmods)
        mode = os.environ.get("NMHIP_SPLIT", "auto")
        if mode == "0" or M < 2 or self.wide or any(len(j.kmods) != M for j in self.jobs):
            return 1
        fits = (len(self.jobs) + 7) // 8 * 8 * M <= self._cus
        return M if fits else 1

    def rowsplit_k(self, mixed: bool = False) -> int:
        """Row slices per (model, modality) for a training launch (nm_launch_rowsplit): the largest k in {4, 2} for which
        all ceil(groups / 8) * 8 * k workgroups are resident at once (groups = the (model, modality) pairs of the set), 1 if
        the set is too large for that or a model needs the whole batch in one workgroup.  NMHIP_ROWSPLIT = 0 switches it
        off, 2 / 4 cap k.  mixed=False (what train() / grads() ask): a set whose models differ in their number of
        modalities keeps k = 1; mixed=True: such a set counts too (one launch for a grid of one- and several-modality
        models: nm_launch_rowsplit_mixed, train(n, rowsplit=k))."""
        mode = os.environ.get("NMHIP_ROWSPLIT", "auto")
        M = len(self.jobs[0].kmods)
        if mode == "0" or self.wide:
            return 1
        groups = ((self._rs_groups() if mixed else len(self.jobs) * M) + 7) // 8 * 8
        kmax = int(mode) if mode in ("2", "4") else 4
        # (the set size first: a full chip's set -- every train() call of the headline -- skips the per-job checks)
        ks = [k for k in (4, 2) if k <= kmax and groups * k <= self._cus and groups <= _lib.NM_RS_MAX_GROUPS]
        if not ks or any((len(j.kmods) != M and not mixed) or not j.rowsplit_ok() for j in self.jobs):
            return 1
        return ks[0]

    def _rs_groups(self) -> int:
        """(model, modality) pairs of the set = groups of a row-split launch before rounding up to a multiple of 8."""
        return sum(len(j.kmods) for j in self.jobs)

    def rowsplit_helpers(self, k: int) -> int:
        """Helper workgroups per (model, modality) of a row-split launch: the CUs the k slices leave idle join the Adam
        sweep (nmhip.h: nm_launch_rowsplit).  A group stays on one XCD (32 CUs); measured (one and five 3 x 379 models,
        k = 4): 6 helpers give all of the gain, beyond 12 the extra arrivals at the hand-off cost what the shorter sweep
        saves -- so at most 12.  NMHIP_RS_HELPERS pins it."""
        env = os.environ.get("NMHIP_RS_HELPERS", "auto")
        groups = (self._rs_groups() + 7) // 8 * 8
        room = max(0, min(self._cus // groups, 32) - k)
        return min(int(env), room) if env != "auto" else min(room, 12)

    def _launch_rowsplit(self, k: int, step0: int, n_steps: int, flags: int, helpers: Optional[int] = None):
        for i, j in enumerate(self.jobs):
            j._ensure_rowsplit(k)
            # (the kernel refuses such a job too, but only after the launch: say which limit, before anything runs)
            if j._rs_ok_version != j._version:
                if self.lib.nm_rowsplit_ok(C.byref(j.struct())) != 0:
                    why = j.rowsplit_limit() or "not a plain cVAE / cVAE_multimodal model on the fused kernel"
                    raise ValueError(f"job {i} of the set cannot run row-split (nm_rowsplit_ok): {why}")
                j._rs_ok_version = j._version
        h = self.rowsplit_helpers(k) if helpers is None else int(helpers)
        # start offsets over ~one step's time -- of the set's largest model -- once the launch fills a good part of the chip
        # (measured: 0.37 ns per parameter and step for one model at k = 4)
        Ms = [len(j.kmods) for j in self.jobs]
        spread = int(max(j.layout.n_params for j in self.jobs) * 0.37e-3 * (4 / k)) if sum(Ms) * k >= 96 else 0
        if all(m == Ms[0] for m in Ms):
            self._issue("nm_launch_rowsplit", k, Ms[0], k, h, step0, n_steps, flags, spread)
        else:        # models that differ in their number of modalities: the group map is built from the per-job counts
            self._issue("nm_launch_rowsplit_mixed", k, (C.c_int * len(Ms))(*Ms), k, h, step0, n_steps, flags, spread)

    def _training_form(self, split: Optional[bool], rowsplit: Optional[int]):
        """The form of a training launch: ("rowsplit", k row slices per (model, modality)), ("split", one workgroup per
        modality) or ("whole", one workgroup per model).  rowsplit=None: rowsplit_k() unless split is given; split=None:
        split_parts()."""
        k = (self.rowsplit_k() if split is None else 1) if rowsplit is None else int(rowsplit)
        if k > 1:
            return "rowsplit", k
        parts = self.split_parts() if split is None else (len(self.jobs[0].kmods) if split else 1)
        return ("split", parts) if parts > 1 else ("whole", 1)

    def _launch_form(self, form, step0: int, n_steps: int, flags: int, helpers: Optional[int], scalar_tr: bool,
                     plain: Optional[bool] = None):
        kind, k = form
        if kind == "rowsplit":
            self._launch_rowsplit(k, step0, n_steps, flags, helpers)
        elif kind == "split":
            self._launch_split(step0, n_steps, flags)
        else:
            self._launch(step0, n_steps, 1, flags, scalar_tr, plain)
            return
        self.last_launch = {"entry": kind, "flags": int(flags), "plain": False}

    def _check_jobs(self, head: Optional[str] = None, caller: str = "", at_step: bool = True) -> int:
        """Preconditions of a launch: every job at the same step (at_step; returned) and, for a head model's step
        (head = "regression" / "endtoend"), jobs of that kind with their targets set and the same batches per epoch."""
        step0 = self.jobs[0].step
        for j in self.jobs:
            if head == "regression" and (j.spec.kind != "regression" or j.fi_target is None):
                raise ValueError(f"{caller} needs regression jobs with fi_target set")
            if head == "endtoend" and (j.spec.kind != "endtoend" or not j.spec.classifier_layers or j.labels is None):
                raise ValueError(f"{caller} needs end-to-end jobs with a classifier and labels set")
            if at_step and j.step != step0:
                raise ValueError("jobs of one set must be at the same step")
        if head is not None and any(j.batches_per_epoch != self.jobs[0].batches_per_epoch for j in self.jobs):
            raise ValueError("jobs of one set must have the same number of batches")
        return step0

    def _advance(self, n_steps: int):
        for j in self.jobs:
            j.step += n_steps
            j.t += n_steps

    def train(self, n_steps: int, scalar_tr: bool = False, profile: bool = False, split: Optional[bool] = None,
              rowsplit: Optional[int] = None, helpers: Optional[int] = None, plain: Optional[bool] = None):
        """n_steps fused train steps per job in ONE launch (forward + ELBO + backward + Adam).  Small sets put several
        workgroups behind a model: k row slices per (model, modality) (rowsplit=None: rowsplit_k(); results agree with the
        one-workgroup launch to fp32 summation order), else one workgroup per modality (split=None: automatically;
        bit-identical to the one-workgroup launch).  scalar_tr: the whole-batch launch on the scalar-loader kernel.
        plain: the one-workgroup launch on the plain-training kernel (None: when every job passes plain_ok(); False: never;
        bit-identical either way), see _launch."""
        step0 = self._check_jobs()
        flags = _lib.NM_F_BACKWARD | _lib.NM_F_ADAM | (_lib.NM_F_PROFILE if profile else 0)
        form = ("whole", 1) if scalar_tr else self._training_form(split, rowsplit)
        self._launch_form(form, step0, n_steps, flags, helpers, scalar_tr, plain)
        self._advance(n_steps)

    def grads(self, step: Optional[int] = None, export: bool = True, scalar_tr: bool = False, split: bool = False,
              rowsplit: int = 1, helpers: Optional[int] = None):
        """forward + loss + backward for one step; gradients land in job.grads (no update)."""
        s = self.jobs[0].step if step is None else step
        flags = _lib.NM_F_BACKWARD | _lib.NM_F_GRADS | (_lib.NM_F_EXPORT if export else 0)
        self._launch_form(self._training_form(split, rowsplit), s, 1, flags, helpers, scalar_tr)

    def devpass_ok(self) -> bool:
        """Can the set's deviation pass run on the compact kernel (nm_devpass: 128-row tiles, two workgroups per CU)?
        The conditions of nm_devpass_ok, read off the jobs (building 256 descriptors per launch to ask the library would
        cost more than the pass; tests/test_cabi_cpu.py holds the two to each other)."""
        if self.wide or os.environ.get("NMHIP_DEVPASS", "1") == "0":
            return False
        return all(j.devpass_ok() for j in self.jobs)

    def devpass_multi_ok(self) -> bool:
        """Can the set's multi-expert reconstruction / deviation pass run on the compact kernel (nm_devpass_multi)?  The
        conditions of nm_devpass_multi_ok, read off the jobs as in devpass_ok (tests/test_cabi_devpass_multi_cpu.py holds
        the two to each other); NMHIP_DEVPASS=0 switches both compact kernels off."""
        if self.wide or os.environ.get("NMHIP_DEVPASS", "1") == "0":
            return False
        return all(j.devpass_multi_ok() for j in self.jobs)

    def devpass_multi_pick(self) -> bool:
        """The automatic pick of nm_devpass_multi for this set: devpass_multi_ok() and a shape class in which the compact
        kernel's slowest measured repeat beat the general kernel's fastest (DEVPASS_MULTI_AUTO).
        NMHIP_DEVPASS_MULTI=1 / 0 forces the pick on (where the set passes devpass_multi_ok) / off."""
        env = os.environ.get("NMHIP_DEVPASS_MULTI", "auto")
        if env == "0" or not self.devpass_multi_ok():
            return False
        return env == "1" or all(DEVPASS_MULTI_AUTO.get(len(j.kmods), False) for j in self.jobs)

    def forward(self, tile0: int = 0, n_tiles: Optional[int] = None, loss: bool = True, trace: bool = False,
                compact: Optional[bool] = None):
        """forward-only over row tiles (one workgroup per (job, 256-row tile)); fills the exports.  loss=False: only the
        per-ROI / per-subject deviations and the reconstruction are wanted (the deviation pass of
        ..._regression.py:163-192, pred_recon + reconstruction_deviation_multimodal of ..._test_cvae_supervised.py:112-113)
        -- sets of one-expert models (nm_devpass) and sets of several-expert models (nm_devpass_multi) then run on the
        compact kernels, two workgroups of 128 rows per CU.  compact (several-expert sets): None = the automatic pick
        (devpass_multi_pick), True = insist on nm_devpass_multi (ValueError if a job of the set cannot run there), False =
        the general kernel.  trace: the compact kernel records its phase cycles (nm_trace_read_dv)."""
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        if not loss and self.devpass_ok():
            self._issue("nm_devpass", 1, tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)
            return
        if compact and (loss or not self.devpass_multi_ok()):
            raise ValueError("compact=True: the set cannot run on nm_devpass_multi (loss wanted, latent exports on, "
                             "NMHIP_DEVPASS=0, or a shape nm_devpass_multi_ok refuses)")
        if not loss and (compact or (compact is None and self.devpass_multi_pick())):
            # (one workspace tile per 256-row batch: the two 128-row workgroups of a batch share it on disjoint rows)
            self._issue("nm_devpass_multi", nt, tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)
            return
        self._launch(tile0, 1, nt, _lib.NM_F_EXPORT)

    def _subsets_refusal(self) -> Optional[str]:
        """Why the set cannot run the modality-subset pass (nm_devpass_subsets_ok asked of every job's descriptor, once per
        state of the descriptor); None: it can."""
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if getattr(j, "_sub_ok_version", None) == j._version:
                continue
            st = self.lib.nm_devpass_subsets_ok(C.byref(j.struct()))
            if st != 0:
                s = j.spec
                return (f"job {i}: nm_devpass_subsets_ok refuses it with status {st} "
                        f"({self.lib.nm_status_string(st).decode()}): kind {s.kind!r}, {s.M} modalities of which "
                        f"{len(j.kmods)} in the kernel, hidden {list(s.hidden)}, latent {s.latent}, private {s.n_private}, "
                        f"tc_weight {j.tc_weight} -- the pass takes 2..{_lib.NM_MAX_EXP} experts, first hidden width <= 112, "
                        f"latent rounded to 16 <= 32, no end-to-end trunk")
            j._sub_ok_version = j._version
        return None

    def _present_rows(self, present):
        """present of forward_subsets -> per job a list of per-entry uint8 device tensors [rows_alloc] (or None)."""
        if present is None:
            return [None] * len(self.jobs)
        per_job = list(present) if isinstance(present, (list, tuple)) else [present] * len(self.jobs)
        if len(per_job) != len(self.jobs):
            raise ValueError(f"present: one entry per job ({len(self.jobs)}), got {len(per_job)}")
        out = []
        for j, p in zip(self.jobs, per_job):
            ns, N, ra = len(j.sub_masks), j.tables[0].N, j.tables[0].rows_alloc
            per_sub = list(p) if isinstance(p, (list, tuple)) else [p] * ns
            if len(per_sub) != ns:
                raise ValueError(f"present: one entry per subset ({ns}), got {len(per_sub)}")
            row, cache = [], {}
            for q in per_sub:
                if q is None:
                    row.append(None)
                    continue
                if id(q) not in cache:
                    t = torch.as_tensor(np.asarray(q) if not torch.is_tensor(q) else q).reshape(-1)
                    if t.numel() != N:
                        raise ValueError(f"present has {t.numel()} values for {N} table rows")
                    if t.dtype == torch.bool or t.is_floating_point() or int(t.min()) < 0 or int(t.max()) >= (1 << len(j.kmods)):
                        raise ValueError(f"present: one integer per row, bit m set where expert m was observed "
                                         f"(0..{(1 << len(j.kmods)) - 1})")
                    buf = torch.zeros(ra, dtype=torch.uint8, device=self.device)
                    buf[:N] = t.to(device=self.device, dtype=torch.uint8)
                    cache[id(q)] = buf
                row.append(cache[id(q)])
            out.append(row)
        return out

    def forward_subsets(self, present=None, tile0: int = 0, n_tiles: Optional[int] = None, trace: bool = False):
        """The modality-subset pass (nm_devpass_subsets): every expert's encoder once per 128-row tile, then per subset of
        Job.enable_subset_exports the fusion of that subset's experts, the latent draw -- the full pass's draw of the row,
        the same for every subset -- and the decoders the subset exports, into job.sub_loc / sub_sqerr / sub_rowdev.  All
        jobs of the set in one launch; they must list the same number of subsets.  present: which experts each row has
        observed -- one integer per table row, bit m for expert m -- as one array (every job and subset), a list per job, or
        per job a list per subset (None entries: all observed); row r of a subset then fuses the subset's experts that r
        has observed, a row with none of them comes back as NaN, and so do out_sqerr / out_rowdev of a modality the row has
        not observed (its reconstruction is the imputation).  A set holding a job the kernel does not take (general-shape
        path, first hidden width > 112, latent rounded to 16 > 32, an end-to-end trunk, one expert) raises ValueError
        naming the refusal.  trace: the kernel records its phase cycles (nm_trace_read_dv)."""
        if any(j.sub_masks is None for j in self.jobs):
            raise ValueError("forward_subsets: Job.enable_subset_exports() first, on every job of the set")
        ns = len(self.jobs[0].sub_masks)
        if any(len(j.sub_masks) != ns for j in self.jobs):
            raise ValueError("forward_subsets: the jobs of one set must list the same number of subsets")
        why = self._subsets_refusal()
        if why is not None:
            raise ValueError("forward_subsets: the set cannot run on nm_devpass_subsets: " + why)
        # the table on the device: rebuilt when a job's descriptor (and with it, maybe, its subset buffers) changed or presence
        # bytes are handed in; kept until then -- the launch reads it, and the presence bytes, in stream order
        sig = tuple(j._version for j in self.jobs) if present is None else None
        if sig is None or getattr(self, "_sub_sig", None) != sig:
            rows = self._present_rows(present)
            table = [e for j, p in zip(self.jobs, rows) for e in j.subset_structs(p)]
            arr = (_lib.NmSubset * len(table))(*table)
            self._sub_keep = (torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), rows)
            self._sub_sig = sig
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        self._issue("nm_devpass_subsets", nt, self._sub_keep[0].data_ptr(), ns, tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)

    def _draws_refusal(self) -> Optional[str]:
        """Why the set cannot run the posterior-predictive pass (nm_devpass_draws_ok asked of every job's descriptor, once per
        state of the descriptor); None: it can."""
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if getattr(j, "_draws_ok_version", None) == j._version:
                continue
            st = self.lib.nm_devpass_draws_ok(C.byref(j.struct()))
            if st != 0:
                s = j.spec
                return (f"job {i}: nm_devpass_draws_ok refuses it with status {st} "
                        f"({self.lib.nm_status_string(st).decode()}): kind {s.kind!r}, {s.M} modalities of which "
                        f"{len(j.kmods)} in the kernel, hidden {list(s.hidden)}, latent {s.latent}, private {s.n_private}, "
                        f"tc_weight {j.tc_weight} -- the pass takes 1..{_lib.NM_MAX_EXP} experts, first hidden width <= 112, "
                        f"latent rounded to 16 <= 32, Gaussian output, no end-to-end trunk")
            j._draws_ok_version = j._version
        return None

    def forward_draws(self, tile0: int = 0, n_tiles: Optional[int] = None, trace: bool = False):
        """The posterior-predictive pass (nm_devpass_draws): every expert's encoder once per 128-row tile, then per draw of
        Job.enable_predictive_exports the fusion, the latent draw and every decoder, the S reconstructions of an element
        folded on the device into job.pred_mean / pred_var / pred_msq / pred_z and the row means pred_rowdev / pred_rowz2.
        All jobs of the set in one launch; they must ask for the same number of draws.  A set holding a job the kernel does
        not take (general-shape path, first hidden width > 112, latent rounded to 16 > 32, an end-to-end trunk, a
        non-Gaussian output) raises ValueError naming the refusal.  trace: the kernel records its phase cycles
        (nm_trace_read_dv)."""
        if any(getattr(j, "n_draws", None) is None for j in self.jobs):
            raise ValueError("forward_draws: Job.enable_predictive_exports() first, on every job of the set")
        S = self.jobs[0].n_draws
        if any(j.n_draws != S for j in self.jobs):
            raise ValueError("forward_draws: the jobs of one set must ask for the same number of draws")
        why = self._draws_refusal()
        if why is not None:
            raise ValueError("forward_draws: the set cannot run on nm_devpass_draws: " + why)
        # the two tables on the device: rebuilt when a job's descriptor (and with it, maybe, its predictive buffers) changed; kept
        # until then -- the launch reads them in stream order
        sig = tuple(j._version for j in self.jobs)
        if getattr(self, "_draw_sig", None) != sig:
            rows = [j.pred_structs() for j in self.jobs]
            draws = (_lib.NmDraw * (S * len(rows)))(*[d for dr, _ in rows for d in dr])
            preds = (_lib.NmPred * len(rows))(*[p for _, p in rows])
            self._draw_keep = (torch.frombuffer(bytearray(bytes(draws)), dtype=torch.uint8).to(self.device),
                               torch.frombuffer(bytearray(bytes(preds)), dtype=torch.uint8).to(self.device))
            self._draw_sig = sig
        for j in self.jobs:
            j.refresh_noise_var()
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        self._issue("nm_devpass_draws", nt, self._draw_keep[0].data_ptr(), S, self._draw_keep[1].data_ptr(), tile0 * 2, nt * 2,
                    _lib.NM_F_TRACE if trace else 0)

    def forward_loglik(self, tile0: int = 0, n_tiles: Optional[int] = None, trace: bool = False):
        """The likelihood pass (nm_devpass_iw): every expert's encoder once per 128-row tile, then per draw of
        Job.enable_likelihood_exports the fusion, the latent draw and every decoder of the request, the importance weights
        log w_s = log p(x | z_s, c) + log p(z_s) - log q(z_s | x, c) folded per subject on the device into job.iw_row
        (metrics.LOGLIK_ROW_COLUMNS: log p(x | c), ELBO, effective sample size, ...) and job.iw_recon_ll.  All jobs of the set
        in one launch; they must ask for the same number of draws.  A set holding a job the kernel does not take raises
        ValueError naming the refusal, as forward_draws does."""
        if any(getattr(j, "iw_draws", None) is None for j in self.jobs):
            raise ValueError("forward_loglik: Job.enable_likelihood_exports() first, on every job of the set")
        S = self.jobs[0].iw_draws
        if any(j.iw_draws != S for j in self.jobs):
            raise ValueError("forward_loglik: the jobs of one set must ask for the same number of draws")
        why = self._draws_refusal()                 # (nm_devpass_iw_ok is nm_devpass_draws_ok: one domain)
        if why is not None:
            raise ValueError("forward_loglik: the set cannot run on nm_devpass_iw: " + why)
        changed = [j.refresh_likelihood_constants() for j in self.jobs]
        sig = tuple(j._version for j in self.jobs)
        if getattr(self, "_iw_sig", None) != sig or any(changed):
            rows = [j.iw_structs() for j in self.jobs]
            for i, (j, (_, q)) in enumerate(zip(self.jobs, rows)):
                st = self.lib.nm_iw_check(C.byref(j.struct()), C.byref(q))
                if st != 0:
                    raise ValueError(f"forward_loglik: job {i}: nm_iw_check refuses the request with status {st} "
                                     f"({self.lib.nm_status_string(st).decode()})")
            draws = (_lib.NmDraw * (S * len(rows)))(*[d for dr, _ in rows for d in dr])
            reqs = (_lib.NmIw * len(rows))(*[q for _, q in rows])
            self._iw_keep = (torch.frombuffer(bytearray(bytes(draws)), dtype=torch.uint8).to(self.device),
                             torch.frombuffer(bytearray(bytes(reqs)), dtype=torch.uint8).to(self.device))
            self._iw_sig = sig
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        self._issue("nm_devpass_iw", nt, self._iw_keep[0].data_ptr(), S, self._iw_keep[1].data_ptr(), tile0 * 2, nt * 2,
                    _lib.NM_F_TRACE if trace else 0)

    def latent_ok(self) -> bool:
        """Can the set's joint latent statistics come from the encoder-only kernel (nm_latent_pass)?  The conditions of
        nm_latent_pass_ok, read off the jobs as in devpass_ok (tests/test_cabi_latent_cpu.py holds the two to each other);
        NMHIP_LATENT=0 switches the kernel off."""
        if self.wide or os.environ.get("NMHIP_LATENT", "1") == "0":
            return False
        return all(j.latent_ok() for j in self.jobs)

    def latent_pick(self) -> bool:
        """The automatic pick of nm_latent_pass for this set: latent_ok() and a shape class in which the encoder-only
        kernel's slowest measured repeat beat the general kernel's fastest (LATENT_AUTO)."""
        return self.latent_ok() and all(LATENT_AUTO.get(len(j.kmods), False) for j in self.jobs)

    def latent(self, tile0: int = 0, n_tiles: Optional[int] = None, compact: Optional[bool] = None, trace: bool = False):
        """The joint posterior of every row -- out_mu / out_logvar of every job, what cVAE.pred_latent returns
        (cVAE.py:539-545) -- over row tiles.  Through the encoder-only kernel (nm_latent_pass: 128-row tiles, two workgroups
        per CU, no draw, no decoder) where every job passes latent_ok(); else through the general forward kernel, which
        computes the decoders as well.  compact: None = the automatic pick (latent_pick), True = insist on nm_latent_pass
        (ValueError with the reason if the set cannot run there), False = the general kernel.  A job whose latent exports
        are off gets them switched on (set_latent_exports).  trace: nm_latent_pass records its phase cycles
        (nm_trace_read_dv)."""
        for j in self.jobs:
            if j.out_mu is None or j.out_logvar is None:
                j.set_latent_exports(True)
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        if compact and not self.latent_ok():
            raise ValueError("compact=True: the set cannot run on nm_latent_pass: " + self._latent_refusal())
        if compact or (compact is None and self.latent_pick()):
            # (several experts: one workspace tile per 256-row batch, shared by the batch's two 128-row workgroups)
            ws_tiles = nt if any(len(j.kmods) > 1 for j in self.jobs) else 1
            self._issue("nm_latent_pass", ws_tiles, tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)
            return
        self._launch(tile0, 1, nt, _lib.NM_F_EXPORT)

    def _latent_refusal(self) -> str:
        if os.environ.get("NMHIP_LATENT", "1") == "0":
            return "NMHIP_LATENT=0"
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if not j.latent_ok():
                s = j.spec
                return (f"job {i}: nm_latent_pass_ok refuses its shape (kind {s.kind!r}, {s.M} modalities of which "
                        f"{len(j.kmods)} in the kernel, hidden {list(s.hidden)}, latent {s.latent}, private {s.n_private}, "
                        f"tc_weight {j.tc_weight})")
        return "nothing"

    def decode_ok(self) -> bool:
        """Can the set's decoders run on the decoder-only kernel (nm_decode_pass)?  The conditions of nm_decode_pass_ok, read
        off the jobs as in latent_ok (tests/test_cabi_decode_cpu.py holds the two to each other); NMHIP_DECODE=0 switches
        the kernel off."""
        if self.wide or os.environ.get("NMHIP_DECODE", "1") == "0":
            return False
        return all(j.decode_ok() for j in self.jobs)

    def decode_pick(self) -> bool:
        """The automatic route of the drop-in classes' decode(z, c, m) through nm_decode_pass: decode_ok() and a shape class in
        which the decoder-only kernel's slowest measured repeat beat today's route's fastest (DECODE_AUTO, DESIGN.md
        section 4b).  NMHIP_DECODE=1 forces the route on where the set passes decode_ok()."""
        if not self.decode_ok():
            return False
        return os.environ.get("NMHIP_DECODE", "auto") == "1" or all(DECODE_AUTO.get(len(j.kmods), False) for j in self.jobs)

    def decode(self, tile0: int = 0, n_tiles: Optional[int] = None, trace: bool = False):
        """The decoder pass (nm_decode_pass): every job's request (Job.enable_decode_exports / set_decode_inputs) -- latent
        rows decoded under their own covariates or under every cell of a covariate grid -- in ONE launch, into job.dec_loc /
        dec_sqerr / dec_rowdev.  The requests may differ in height and in their number of cells: the grid is as tall as the
        tallest, n_tiles (256-row tiles, from tile0) defaults to that.  A set holding a job the kernel does not take
        (general-shape path, first hidden width > 112, latent rounded to 16 > 32, an end-to-end trunk, a non-Gaussian
        output) or NMHIP_DECODE=0 raises ValueError naming the refusal.  trace: the kernel records its phase cycles
        (nm_trace_read_dv)."""
        if any(j.dec_rows is None or j.dec_z is None for j in self.jobs):
            raise ValueError("decode: Job.enable_decode_exports() and set_decode_inputs() first, on every job of the set")
        why = self._decode_refusal()
        if why is not None:
            raise ValueError("decode: the set cannot run on nm_decode_pass: " + why)
        # the request table on the device: rebuilt when a job's request changed; kept until then -- the launch reads it in
        # stream order
        sig = tuple(j._dec_epoch for j in self.jobs)
        if getattr(self, "_dec_sig", None) != sig:
            arr = (_lib.NmDecode * len(self.jobs))(*[j.decode_struct() for j in self.jobs])
            self._dec_keep = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
            self._dec_sig = sig
        nt = max(j.dec_rows_alloc for j in self.jobs) // BATCH if n_tiles is None else n_tiles
        self._issue("nm_decode_pass", 1, self._dec_keep.data_ptr(), tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)

    def _decode_refusal(self) -> Optional[str]:
        """Why the set cannot run the decoder pass; None: it can."""
        if os.environ.get("NMHIP_DECODE", "1") == "0":
            return "NMHIP_DECODE=0"
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if not j.decode_ok():
                s = j.spec
                return (f"job {i}: nm_decode_pass_ok refuses its shape (kind {s.kind!r}, {s.M} modalities of which "
                        f"{len(j.kmods)} in the kernel, hidden {list(s.hidden)}, latent {s.latent}, private {s.n_private}, "
                        f"tc_weight {j.tc_weight})")
        return None

    def chart_ok(self) -> bool:
        """Can the set's charts run on nm_chart_pass?  decode_ok(): the same kernel code, the same switch (NMHIP_DECODE=0)."""
        return self.decode_ok()

    def chart_pick(self) -> bool:
        """The automatic route of normative_trajectory through the chart pass: chart_ok() and a shape class CHART_AUTO has
        switched on; NMHIP_CHART=1 forces the route on where the set passes chart_ok()."""
        if not self.chart_ok():
            return False
        return os.environ.get("NMHIP_CHART", "auto") == "1" or all(CHART_AUTO.get(len(j.kmods), False) for j in self.jobs)

    def chart(self, tile0: int = 0, n_tiles: Optional[int] = None):
        """The chart pass (nm_chart_pass): every job's request (Job.enable_chart_exports / set_chart_inputs) in ONE launch --
        a workgroup per (128-row tile, cell, decoder), the per-cell moments folded in the kernel, then the merge of the
        tile partials -- into job.chart[m] ([n_cells, D, 4] fp64: metrics.CHART_COLUMNS) and, where asked for, job.chart_loc.
        The requests may differ in height and in their number of cells.  n_tiles (256-row tiles, from tile0) defaults to
        the tallest request; the merge runs only from tile0 = 0 and for requests the launch covers.  A set the decoder pass
        refuses raises ValueError in _decode_refusal's wording."""
        if any(j.chart_rows is None or j.chart_z is None for j in self.jobs):
            raise ValueError("chart: Job.enable_chart_exports() and set_chart_inputs() first, on every job of the set")
        why = self._decode_refusal()
        if why is not None:
            raise ValueError("chart: the set cannot run on nm_chart_pass: " + why)
        sig = tuple(j._chart_epoch for j in self.jobs)
        if getattr(self, "_chart_sig", None) != sig:
            arr = (_lib.NmChart * len(self.jobs))(*[j.chart_struct() for j in self.jobs])
            self._chart_keep = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
            self._chart_sig = sig
        nt = max(j.chart_rows_alloc for j in self.jobs) // BATCH if n_tiles is None else n_tiles
        self._issue("nm_chart_pass", 1, self._chart_keep.data_ptr(), tile0 * 2, nt * 2, max(j.chart_cells for j in self.jobs), 0)

    # -- the end-to-end model's evaluation ---------------------------------------------------------
    def e2e_ok(self) -> bool:
        """Can the set's evaluation run on nm_e2e_pass (every job passes the library's nm_e2e_pass_ok)?  NMHIP_E2E=0
        switches the kernel off."""
        if self.wide or os.environ.get("NMHIP_E2E", "auto") == "0":
            return False
        return all(j.e2e_ok() for j in self.jobs)

    def e2e_pick(self) -> bool:
        """The automatic route of forward_endtoend: e2e_ok() and a class of sets E2E_AUTO has switched on (by the number of
        experts); NMHIP_E2E=1 forces the pass on where the set passes e2e_ok()."""
        if not self.e2e_ok():
            return False
        return os.environ.get("NMHIP_E2E", "auto") == "1" or all(E2E_AUTO.get(j.spec.M, False) for j in self.jobs)

    def _e2e_refusal(self) -> str:
        if os.environ.get("NMHIP_E2E", "auto") == "0":
            return "NMHIP_E2E=0"
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if not j.e2e_ok():
                s = j.spec
                return (f"job {i}: nm_e2e_pass_ok refuses its shape (kind {s.kind!r}, {s.M} experts, {len(j.kmods)} decoders, "
                        f"hidden {list(s.hidden)}, latent {s.latent}, classifier {list(s.classifier_layers or ())}, "
                        f"{s.num_classes} classes)")
        return "nothing"

    def forward_endtoend(self, latent: str = "mean", compact: Optional[bool] = None, tile0: int = 0, n_tiles: Optional[int] = None,
                         trace: bool = False, logits_only: bool = False):
        """The evaluation of cVAE_multimodal_endtoend jobs over row tiles, all jobs of the set at once: the joint posterior,
        the latent (latent="mean": z = mu_joint; "draw": the forward kernel's draw of every row, or the job's injected eps),
        the classifier in eval mode (on mu_joint where job.cls_use_mu, else on z), both decoder banks, and per subject
        job.e2e_row (metrics.ENDTOEND_ROW_COLUMNS) -- into the buffers of Job.enable_endtoend_exports.  compact: None = the
        automatic pick (e2e_pick); True = insist on nm_e2e_pass, one launch (ValueError naming the refusal if the set cannot
        run there); False = the two-launch route, forward(loss=False) + head_classifier + the row table folded with fp32
        torch operations in the kernel's order -- also the route of every set nm_e2e_pass_ok refuses (a trunk on the
        general-shape path, a classifier with blocks wider than 128).  Both routes leave cls_train off (model.eval()); the
        running statistics are never written.  logits_only: this call wants out_logits (and the latent exports) alone, whatever
        buffers the jobs hold -- the pass then runs no decoder and writes no row table, the two-launch route skips the fold.
        The two-launch route keeps the jobs' descriptors as they are wherever it can: with latent="draw" nothing of a job
        changes; with "mean" a job whose eps is not already the all-zero draw gets it installed for the call (a device
        buffer kept with the job) and its own back afterwards, which costs that job a descriptor upload."""
        if latent not in ("mean", "draw"):
            raise ValueError("latent: 'mean' or 'draw'")
        if any(not getattr(j, "e2e_enabled", False) for j in self.jobs):
            raise ValueError("forward_endtoend: Job.enable_endtoend_exports() first, on every job of the set")
        if compact and not self.e2e_ok():
            raise ValueError("compact=True: the set cannot run on nm_e2e_pass: " + self._e2e_refusal())
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        for j in self.jobs:
            j._e2e_require_alpha("forward_endtoend")
            if j.cls_train:
                j.cls_train = False
                j._version += 1
        if compact or (compact is None and self.e2e_pick()):
            sig = (latent, logits_only, tuple(j._version for j in self.jobs))
            if getattr(self, "_e2e_sig", None) != sig:
                rows = [j.e2e_struct(latent == "mean") for j in self.jobs]
                for q in rows:
                    if logits_only:
                        q.row, q.want_mask = None, 0
                reqs = (_lib.NmE2e * len(self.jobs))(*rows)
                self._e2e_keep = torch.frombuffer(bytearray(bytes(reqs)), dtype=torch.uint8).to(self.device)
                self._e2e_sig = sig
            # (one workspace tile per 256-row batch: the two 128-row workgroups of a batch share it on disjoint rows)
            self._issue("nm_e2e_pass", nt, self._e2e_keep.data_ptr(), tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)
            return
        # ---- the two-launch route ----
        stash = []
        for j in self.jobs:
            held = None
            # an all-zero draw: z = mu_joint + 0 * exp(logvar / 2) (not needed where only a classifier on mu is read)
            if latent == "mean" and not (logits_only and j.cls_use_mu):
                zero = getattr(j, "_e2e_zero_eps", None)
                if zero is None or zero.shape[2] != j.spec.latent:
                    zero = j._e2e_zero_eps = torch.zeros(1, BATCH, j.spec.latent, device=j.device)
                if j.eps is not zero:
                    held = (j.eps, j.eps_cap)
                    j.eps, j.eps_cap = zero, 1
                    j._version += 1
            rowdev = None
            if not logits_only and j.e2e_row is not None and any(o is None for o in j.out_rowdev):
                rowdev = list(j.out_rowdev)
                j.out_rowdev = [o if o is not None else torch.zeros(j.tables[0].rows_alloc, device=j.device) for o in j.out_rowdev]
                j._version += 1
            stash.append((held, rowdev))
        self.forward(tile0=tile0, n_tiles=nt, loss=False, compact=False)
        self.head_classifier(backward=False, tile0=tile0, n_tiles=nt)
        for j, (held, rowdev) in zip(self.jobs, stash):
            r0, r1 = tile0 * BATCH, min((tile0 + nt) * BATCH, j.tables[0].rows_alloc)
            if not logits_only and j.e2e_row is not None:
                _endtoend_row_fold(j, r0, r1)
            if j.tables[0].N < r1:                      # rows past the table: zeros, as from the pass
                for t in (j.out_mu, j.out_logvar, j.out_z, j.out_logits):
                    if t is not None:
                        t[max(r0, j.tables[0].N):r1] = 0.0
            if held is not None:
                j.eps, j.eps_cap = held
                j._version += 1
            if rowdev is not None:
                j.out_rowdev = rowdev
                j._version += 1

    # -- the regression model's evaluation ---------------------------------------------------------
    def fi_ok(self) -> bool:
        """Can the set's FI evaluation run on nm_fi_pass (every job passes the library's nm_fi_pass_ok)?  NMHIP_FI=0 switches
        the kernel off."""
        if self.wide or os.environ.get("NMHIP_FI", "auto") == "0":
            return False
        return all(j.fi_ok() for j in self.jobs)

    def fi_pick(self) -> bool:
        """The automatic route of forward_fi: fi_ok() and a class of sets FI_AUTO has switched on (by the number of experts);
        NMHIP_FI=1 forces the pass on where the set passes fi_ok()."""
        if not self.fi_ok():
            return False
        return os.environ.get("NMHIP_FI", "auto") == "1" or all(FI_AUTO.get(j.spec.M, False) for j in self.jobs)

    def _fi_refusal(self) -> str:
        if os.environ.get("NMHIP_FI", "auto") == "0":
            return "NMHIP_FI=0"
        if self.wide:
            return "general-shape path (a hidden width or latent beyond the fused kernel's tile)"
        for i, j in enumerate(self.jobs):
            if not j.fi_ok():
                s = j.spec
                return (f"job {i}: nm_fi_pass_ok refuses its shape (kind {s.kind!r}, {s.M} experts, {len(j.kmods)} decoders, "
                        f"hidden {list(s.hidden)}, latent {s.latent})")
        return "nothing"

    def forward_fi(self, latent: str = "draw", n_draws: int = 1, seeds=None, eps=None, compact: Optional[bool] = None,
                   tile0: int = 0, n_tiles: Optional[int] = None, trace: bool = False):
        """The evaluation of cVAE_multimodal_regression jobs over row tiles, all jobs of the set at once: the joint posterior,
        S = n_draws latents per row (latent="draw": with n_draws == 1 and neither seeds nor eps the forward kernel's own draw
        of every row -- job.seed or the job's injected eps; otherwise one generator key per draw, seeds or
        draw_seeds(job.seed, S), or eps, a list of S tensors in the layout set_eps takes; latent="mean": z = mu_joint, one
        draw), every decoder and the regressor on the residuals, and per subject job.fi_row (metrics.FI_ROW_COLUMNS) -- into the
        buffers of Job.enable_fi_exports; out_fi_pred, the latent and the decoder exports hold draw 0.  compact: None = the
        automatic pick (fi_pick); True = insist on nm_fi_pass, one launch (ValueError naming the refusal if the set cannot run
        there); False = the two-launch route per draw, the general forward kernel with exports + head_regression, the row
        table folded with fp32 torch operations in the kernel's order -- also the route of every set nm_fi_pass_ok refuses
        (a trunk on the general-shape path, a latent above 32).  The two-launch route installs each draw's key or eps (for
        "mean": an all-zero eps) in the job for its launches and puts the job's own back afterwards."""
        if latent not in ("mean", "draw"):
            raise ValueError("latent: 'mean' or 'draw'")
        if any(not getattr(j, "fi_enabled", False) for j in self.jobs):
            raise ValueError("forward_fi: Job.enable_fi_exports() first, on every job of the set")
        S = int(n_draws)
        if latent == "mean" and (S != 1 or seeds is not None or eps is not None):
            raise ValueError(f"forward_fi: latent='mean' is one deterministic pass (n_draws = 1, no seeds, no eps), got n_draws = {n_draws}")
        if compact and not self.fi_ok():
            raise ValueError("compact=True: the set cannot run on nm_fi_pass: " + self._fi_refusal())
        own = latent == "mean" or (S == 1 and seeds is None and eps is None)      # the job's own seed / eps: no draw table
        caps = [j.eps_cap for j in self.jobs]
        reqs = [None if own else j._draw_request(S, seeds, eps, _lib.NM_MAX_DRAWS) for j in self.jobs]
        for j, cap in zip(self.jobs, caps):
            if j.eps_cap != cap:                         # (injected draws index as the job's own eps would)
                j._version += 1
        nt = self.jobs[0].tables[0].n_tiles if n_tiles is None else n_tiles
        try:
            if compact or (compact is None and self.fi_pick()):
                structs = [j.fi_struct(latent == "mean", S) for j in self.jobs]
                sig = (latent, S, own, tuple(j._version for j in self.jobs),
                       tuple((tuple(r[1]), tuple(e.data_ptr() for e in r[2]) if r[2] is not None else None) if r else None for r in reqs),
                       tuple((q.row, q.fi_draws) for q in structs))
                if getattr(self, "_fi_sig", None) != sig:
                    arr = (_lib.NmFi * len(structs))(*structs)
                    draws = None
                    if not own:
                        flat = []
                        for _, keys, ep in reqs:
                            for s in range(S):
                                d = _lib.NmDraw()
                                d.seed, d.eps = keys[s], (ep[s].data_ptr() if ep is not None else None)
                                flat.append(d)
                        draws = torch.frombuffer(bytearray(bytes((_lib.NmDraw * len(flat))(*flat))), dtype=torch.uint8).to(self.device)
                    self._fi_keep = (torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), draws,
                                     [r[2] for r in reqs if r])
                    self._fi_sig = sig
                # (one workspace tile per 256-row batch: the two 128-row workgroups of a batch share it on disjoint rows)
                self._issue("nm_fi_pass", nt, self._fi_keep[1].data_ptr() if self._fi_keep[1] is not None else 0, S,
                            self._fi_keep[0].data_ptr(), tile0 * 2, nt * 2, _lib.NM_F_TRACE if trace else 0)
                return
            self._forward_fi_two_launch(latent, S, reqs, tile0, nt)
        finally:
            for j, cap in zip(self.jobs, caps):
                if j.eps_cap != cap:
                    j.eps_cap = cap
                    j._version += 1

    def _forward_fi_two_launch(self, latent: str, S: int, reqs, tile0: int, nt: int):
        """forward_fi's two-launch route: per draw the general forward kernel with exports and nm_head_regression; draw 0 runs
        last, so that out_fi_pred, the latent and the decoder exports hold it, as from the pass."""
        stash = []
        for j in self.jobs:
            j.fi_struct(latent == "mean", S)               # (fi_draws for this number of draws)
            held = (j.eps, j.eps_cap, j.seed)
            off = [k for k in range(len(j.kmods)) if not (j.fi_mask >> k) & 1]      # decoders whose exports stay as they are
            bufs = (list(j.out_loc), list(j.out_sqerr), list(j.out_rowdev))
            for k in off:
                j.out_loc[k] = j.out_sqerr[k] = j.out_rowdev[k] = None
            if j.fi_row is not None:
                j.out_rowdev = [o if o is not None else torch.zeros(j.tables[0].rows_alloc, device=j.device) for o in j.out_rowdev]
            stash.append((held, bufs))
        preds = [[None] * S for _ in self.jobs]
        for s in list(range(1, S)) + [0]:
            for j, rq in zip(self.jobs, reqs):
                if latent == "mean":
                    # an all-zero draw: z = mu_joint + 0 * exp(logvar / 2)
                    zero = getattr(j, "_fi_zero_eps", None)
                    if zero is None or zero.shape[2] != j.spec.latent:
                        zero = j._fi_zero_eps = torch.zeros(1, BATCH, j.spec.latent, device=j.device)
                    j.eps, j.eps_cap = zero, 1
                elif rq is not None:
                    if rq[2] is not None:
                        j.eps = rq[2][s]
                    else:
                        j.seed = rq[1][s]
                j._version += 1
            self._launch(tile0, 1, nt, _lib.NM_F_EXPORT)
            self.head_regression(backward=False, tile0=tile0, n_tiles=nt)
            for i, j in enumerate(self.jobs):
                preds[i][s] = j.out_fi_pred.clone() if S > 1 else j.out_fi_pred
        for i, (j, (held, bufs)) in enumerate(zip(self.jobs, stash)):
            r0, r1 = tile0 * BATCH, min((tile0 + nt) * BATCH, j.tables[0].rows_alloc)
            n0 = max(r0, min(j.tables[0].N, r1))
            if j.fi_draws is not None:
                j.fi_draws[r0:r1] = torch.stack(preds[i], dim=1)[r0:r1]
                j.fi_draws[n0:r1] = 0.0
            if j.fi_row is not None:
                _fi_row_fold(j, r0, r1, preds[i])
            for t in (j.out_mu, j.out_logvar, j.out_z, j.out_fi_pred):      # rows past the table: zeros, as from the pass
                if t is not None:
                    t[n0:r1] = 0.0
            j.eps, j.eps_cap, j.seed = held
            j.out_loc, j.out_sqerr, j.out_rowdev = bufs
            j._version += 1

    def latent_stats(self):
        """Per job the column means and population variances of its exported joint mu over the table's rows (the training
        cohort's latent distribution, utils_vae.py:156-157) -- all jobs of the set in ONE launch of nm_latent_stats.
        Returns (mean, var), device tensors [n_jobs, Z]."""
        return latent_stats([j.out_mu[:j.tables[0].N] for j in self._latent_jobs()])

    def latent_scores(self, mean: torch.Tensor, var: torch.Tensor):
        """Per job separate_latent_deviation and latent_deviation (utils_vae.py:155-161) of its exported joint (mu, logvar)
        against row k of mean / var [n_jobs, Z] -- all jobs in ONE launch of nm_latent_score.  Returns (zsep, score): lists
        of device tensors [N_k, Z] / [N_k]."""
        jobs = self._latent_jobs()
        return latent_scores([j.out_mu[:j.tables[0].N] for j in jobs], [j.out_logvar[:j.tables[0].N] for j in jobs], mean, var)

    def _latent_jobs(self):
        if any(j.out_mu is None or j.out_logvar is None for j in self.jobs):
            raise ValueError("latent exports are off: run JobSet.latent() (or forward() with enable_exports(latent=True)) first")
        if any(j.spec.latent != self.jobs[0].spec.latent for j in self.jobs):
            raise ValueError("jobs of one set must have the same latent size")
        return self.jobs

    def head_regression(self, backward: bool, grads: bool = True, adam: bool = False, step: int = 0, tile0: int = 0,
                        n_tiles: int = 1):
        """nm_head_regression on the residual images a preceding forward() / NM_F_EXPORT launch left in job.reg_resid:
        fills out_fi_pred and loss_log[..][NM_LOSS_REG]; with backward also job.reg_dres (d MSE / d x_hat, bf16 chunk
        images) and the regressor's gradients / Adam update (cVAE.py:2309-2346).  Training runs through
        train_regression (one launch for trunk and head)."""
        flags = (_lib.NM_F_BACKWARD if backward else 0) | (_lib.NM_F_GRADS if grads and backward else 0) | \
                (_lib.NM_F_ADAM if adam and backward else 0)
        self._issue("nm_head_regression", max(n_tiles, 1), step, tile0, n_tiles, flags)

    def head_classifier(self, backward: bool, grads: bool = True, adam: bool = False, bn_stats: bool = False,
                        step: int = 0, tile0: int = 0, n_tiles: int = 1):
        """nm_head_classifier on the latent / deviations a preceding NM_F_EXPORT launch exported: fills out_logits
        and loss_log[..][NM_LOSS_CE / NM_LOSS_CONTRAST]; with backward also dz_extra, the hinge row coefficients
        and the classifier's gradients / Adam update (cVAE.py:2004-2018, 2140-2200)."""
        flags = (_lib.NM_F_BACKWARD if backward else 0) | (_lib.NM_F_GRADS if grads and backward else 0) | \
                (_lib.NM_F_ADAM if adam and backward else 0) | (_lib.NM_F_BNSTATS if bn_stats else 0)
        self._issue("nm_head_classifier", max(n_tiles, 1), step, tile0, n_tiles, flags)

    def _train_head(self, step0: int, n_steps: int, flags: int = 0, parts: int = 1):
        """nm_train_steps_head: all n_steps in one persistent launch, the trunk's forward evaluated once per step.
        parts > 1: nm_train_steps_head_split, one workgroup per decoder of every model (head_split_parts)."""
        if parts > 1:
            self._issue("nm_train_steps_head_split", 1, parts, step0, n_steps, flags)
        else:
            self._issue("nm_train_steps_head", 1, step0, n_steps, flags)

    def _head_split_refusal(self, fused: bool = True) -> Optional[str]:
        """Why the set's head models cannot run one workgroup per decoder (nm_train_steps_head_split); None: they can."""
        M = len(self.jobs[0].kmods)
        if self.wide:
            return "a trunk on the general-shape path trains in the three-launch form"
        if not fused:
            return "fused=False asks for the three-launch form"
        if any(w > 128 for j in self.jobs for w in (j.spec.classifier_layers or ())):
            return "a classifier with blocks wider than 128 trains in the three-launch form"
        if any(len(j.kmods) != M for j in self.jobs):
            return "the models of the set differ in their number of decoders"
        if M < 2:
            return "the models have a single decoder"
        if (len(self.jobs) + 7) // 8 * 8 * M > self._cus:
            return (f"{len(self.jobs)} models x {M} workgroups (sets are padded to a multiple of 8 models) exceed the "
                    f"device's {self._cus} CUs: the parts of a model must all be resident at once")
        return None

    def head_split_parts(self, fused: bool = True) -> int:
        """Workgroups per model for a head-model training launch (train_regression / train_endtoend): one per decoder
        (regression: 3; end-to-end: 6, two decoder banks) when split_parts() allows it -- NMHIP_SPLIT, the same number of
        decoders in every model, all workgroups resident at once, not the general-shape path -- and the persistent head
        kernel runs the step at all (fused, one-tile classifier); else 1."""
        parts = self.split_parts()
        if parts < 2 or self._head_split_refusal(fused) is not None:
            return 1
        return parts

    def _head_parts(self, split: Optional[bool], fused: bool = True) -> int:
        """split=None: head_split_parts(); True: insist (ValueError with the reason if the set cannot); False: 1."""
        if split is None:
            return self.head_split_parts(fused)
        if not split:
            return 1
        why = self._head_split_refusal(fused)
        if why is not None:
            raise ValueError(f"split=True: this set cannot run one workgroup per decoder (nm_train_steps_head_split): {why}")
        return len(self.jobs[0].kmods)

    def _head_step(self, head: str, s: int, adam: bool):
        """One head-model step as three launches -- the form a trunk on the general-shape path or a classifier with blocks
        wider than 128 runs in: the trunk's forward with its exports, the head (forward, backward, its Adam update or
        gradients, the extra gradient it hands the trunk), the trunk's backward + Adam / gradients with that gradient."""
        tile0 = s % self.jobs[0].batches_per_epoch
        self._launch(s, 1, 1, _lib.NM_F_EXPORT)
        if head == "regression":
            self.head_regression(backward=True, grads=not adam, adam=adam, step=s, tile0=tile0)
        else:
            self.head_classifier(backward=True, grads=not adam, adam=adam, bn_stats=True, step=s, tile0=tile0)
        self._launch(s, 1, 1, _lib.NM_F_BACKWARD | (_lib.NM_F_ADAM if adam else _lib.NM_F_GRADS))

    def train_endtoend(self, n_steps: int, fused: bool = True, split: Optional[bool] = None):
        """n_steps train steps of cVAE_multimodal_endtoend jobs on the device, no host sync (the loop of
        multimodal_kfold_cvae_nmpmcont.py:257-303): per step (i) forward with latent and per-subject deviations
        exported, (ii) the classifier head: forward (train-mode BatchNorm / Dropout), cross entropy, contrastive
        hinge, backward, its Adam update, d CE / d z and the hinge row coefficients, (iii) the trunk's backward + Adam
        with those extra gradients.  fused (default): one persistent launch for all steps (nm_train_steps_head);
        fused=False: the three-launches-per-step form it replaced (trunk forward twice), kept as a cross-check -- and the
        form a trunk on the general-shape path or a classifier with blocks wider than 128 (-Layers "256 128 64") runs in:
        the persistent head kernel holds the one-tile classifier only.  Small sets run the persistent launch with one
        workgroup per decoder (split=None: head_split_parts(); bit-identical to the one-workgroup launch)."""
        step0 = self._check_jobs("endtoend", "train_endtoend")
        parts = self._head_parts(split, fused)
        for j in self.jobs:
            j.cls_train, j.cls_use_mu = True, False
            j.prepare_classifier()
        tiled_head = any(w > 128 for j in self.jobs for w in j.spec.classifier_layers)
        if fused and not self.wide and not tiled_head:
            self._train_head(step0, n_steps, _lib.NM_F_BNSTATS, parts)
        else:
            for s in range(step0, step0 + n_steps):
                self._head_step("endtoend", s, adam=True)
        self._advance(n_steps)

    def train_regression(self, n_steps: int, split: Optional[bool] = None):
        """n_steps train steps of cVAE_multimodal_regression jobs in one persistent launch, no host sync (the loop of
        multimodal_kfold_train_cvae_supervised_regression.py:112-125): per step (i) the trunk's forward, leaving the
        residuals as bf16 chunk images, (ii) the regressor: forward, MSE, backward, its Adam update, d MSE / d x_hat,
        (iii) the trunk's backward + Adam with that extra gradient (nm_train_steps_head).  A trunk on the general-shape
        path runs the three-launch form (_head_step).  Small sets run the launch with one workgroup per decoder
        (split=None: head_split_parts(); bit-identical to the one-workgroup launch)."""
        step0 = self._check_jobs("regression", "train_regression")
        parts = self._head_parts(split)
        for j in self.jobs:
            j.prepare_regression()
        if self.wide:
            for s in range(step0, step0 + n_steps):
                self._head_step("regression", s, adam=True)
        else:
            self._train_head(step0, n_steps, 0, parts)
        self._advance(n_steps)

    def grads_head(self, step: int = 0, split: bool = False):
        """Gradients of one head-model step's total loss into job.grads, no update (regression sets: the eager facade's
        backward; end-to-end sets: the classifier as the jobs have it set up, running statistics untouched); a trunk on the
        general-shape path or a classifier with blocks wider than 128 runs the three-launch form.  split=True: one
        workgroup per decoder (the same gradients bit for bit); the default stays the one-workgroup launch, the eager
        facade's path."""
        head = "endtoend" if self.jobs[0].spec.kind == "endtoend" else "regression"
        self._check_jobs(head, "grads_head", at_step=False)
        parts = self._head_parts(bool(split))
        if head == "endtoend":
            for j in self.jobs:
                j.prepare_classifier()
        if self.wide or (head == "endtoend" and any(w > 128 for j in self.jobs for w in j.spec.classifier_layers)):
            self._head_step(head, step, adam=False)
        else:
            self._train_head(step, 1, _lib.NM_F_GRADS, parts)

    def losses(self) -> torch.Tensor:
        """[n_jobs, loss_cap, 8] on the host."""
        self.check_split_errors()
        return torch.stack([j.loss_log for j in self.jobs]).cpu()

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def assert_finite(self):
        """Failure detection, once per epoch / run rather than per step (the reference prints NaNs from inside
        its hot loop, cVAE.py:1169-1172): one device reduction over every job's loss ring; raises NmError naming
        the first job whose log holds a non-finite value.  Also the point where a timed-out hand-off of a split
        launch surfaces at the latest (check_split_errors)."""
        self.check_split_errors()
        logs = torch.stack([j.loss_log for j in self.jobs])
        ok = torch.isfinite(logs).flatten(1).all(dim=1)
        if not bool(ok.all()):
            bad = int((~ok).nonzero()[0])
            raise _lib.NmError(f"non-finite loss in job {bad} of {len(self.jobs)} (step {self.jobs[bad].step})")


def _endtoend_row_fold(j: Job, r0: int, r1: int):
    """job.e2e_row over table rows [r0, r1) from the job's exports (out_logits, out_rowdev of every decoder, out_mu,
    out_logvar): nm_e2e_pass' definition (include/nmhip.h) in fp32 torch operations, operation by operation; rows past the
    table's end are zeros."""
    n1 = min(r1, j.tables[0].N)
    j.e2e_row[r0:r1] = 0.0
    if n1 <= r0:
        return
    Cn, Me, Z = j.spec.num_classes, j.spec.M, j.spec.latent
    lg = j.out_logits[r0:n1, :Cn]
    e = torch.exp(lg - lg.max(dim=1, keepdim=True).values)
    sd, sa = e[:, 1].clone(), e[:, 0] + e[:, 1]
    for k in range(2, Cn):
        sd, sa = sd + e[:, k], sa + e[:, k]
    dev = [o[r0:n1] for o in j.out_rowdev]
    dh, dd = dev[0].clone(), dev[Me].clone()
    for m in range(1, Me):
        dh, dd = dh + dev[m], dd + dev[Me + m]
    dh, dd = dh / torch.full_like(dh, Me), dd / torch.full_like(dd, Me)      # (a true division: by a Python scalar torch multiplies by 1 / Me)
    mu, lv = j.out_mu[r0:n1], j.out_logvar[r0:n1]
    t = ((1.0 + lv) - mu * mu) - torch.exp(lv)
    # four interleaved partial sums: columns i, i + 4, ... (Z a multiple of 4: quads 4 i .., 4 (i + 4) ..), (p0 + p1) + (p2 + p3)
    cols = [[z for q in range(i, Z // 4, 4) for z in range(4 * q, 4 * q + 4)] if Z % 4 == 0 else list(range(i, Z, 4)) for i in range(4)]
    parts = []
    for cs in cols:
        p = torch.zeros(n1 - r0, device=t.device)
        for z in cs:
            p = p + t[:, z]
        parts.append(p)
    kl = -0.5 * ((parts[0] + parts[1]) + (parts[2] + parts[3]))
    bad = ~(torch.isfinite(lg).all(dim=1) & torch.isfinite(mu).all(dim=1) & torch.isfinite(lv).all(dim=1))
    for d in dev:
        bad = bad | ~torch.isfinite(d)
    j.e2e_row[r0:n1] = torch.stack([sd / sa, torch.argmax(lg, dim=1).float(), lg[:, 1:].max(dim=1).values - lg[:, 0], dh, dd, dh - dd,
                                    kl, bad.float()], dim=1)


def _fi_row_fold(j: Job, r0: int, r1: int, preds: Sequence[torch.Tensor]):
    """job.fi_row over table rows [r0, r1) from the S predictions of every row (preds[s]: [rows_alloc], s ascending) and the
    job's exports of draw 0 (out_rowdev of every decoder, out_mu, out_logvar): nm_fi_pass' definition (include/nmhip.h) in
    fp32 torch operations, operation by operation; rows past the table's end are zeros.  A job without latent exports gets
    kl = 0 from this route (the statistics never left the forward kernel)."""
    n1 = min(r1, j.tables[0].N)
    j.fi_row[r0:r1] = 0.0
    if n1 <= r0:
        return
    S, M, Z = len(preds), len(j.kmods), j.spec.latent
    p = [q[r0:n1] for q in preds]
    mean, m2, lo, hi = p[0].clone(), torch.zeros_like(p[0]), p[0].clone(), p[0].clone()
    bad = ~torch.isfinite(p[0])
    for s in range(1, S):
        rs = float(np.float32(1.0) / np.float32(s + 1))
        d = p[s] - mean
        mean = mean + d * rs
        m2 = m2 + d * (p[s] - mean)
        lo, hi = torch.fmin(lo, p[s]), torch.fmax(hi, p[s])
        bad = bad | ~torch.isfinite(p[s])
    sd = torch.sqrt(m2 * float(np.float32(1.0) / np.float32(S - 1))) if S > 1 else torch.zeros_like(mean)
    err = mean - j.fi_target[r0:n1] if j.fi_target is not None else torch.zeros_like(mean)
    dev = None
    for o in j.out_rowdev:
        dev = o[r0:n1].clone() if dev is None else dev + o[r0:n1]
        bad = bad | ~torch.isfinite(o[r0:n1])
    dev = dev / torch.full_like(dev, M)                 # (a true division: by a Python scalar torch multiplies by 1 / M)
    kl = torch.zeros_like(mean)
    if j.out_mu is not None and j.out_logvar is not None:
        mu, lv = j.out_mu[r0:n1], j.out_logvar[r0:n1]
        t = ((1.0 + lv) - mu * mu) - torch.exp(lv)
        # four interleaved partial sums, as in _endtoend_row_fold
        cols = [[z for q in range(i, Z // 4, 4) for z in range(4 * q, 4 * q + 4)] if Z % 4 == 0 else list(range(i, Z, 4)) for i in range(4)]
        parts = []
        for cs in cols:
            a = torch.zeros(n1 - r0, device=t.device)
            for z in cs:
                a = a + t[:, z]
            parts.append(a)
        kl = -0.5 * ((parts[0] + parts[1]) + (parts[2] + parts[3]))
        bad = bad | ~(torch.isfinite(mu).all(dim=1) & torch.isfinite(lv).all(dim=1))
    status = bad.float() + (0.0 if j.fi_target is not None else 2.0)
    j.fi_row[r0:n1] = torch.stack([mean, sd, lo, hi, err, dev, kl, status], dim=1)


def _latent_sets(arrays: Sequence[torch.Tensor]):
    """[N_k, Z] fp32 device arrays -> (their rows concatenated, the offsets table on the device, Z)."""
    if not arrays:
        raise ValueError("no set")
    Z = int(arrays[0].shape[1])
    if any(a.dim() != 2 or int(a.shape[1]) != Z for a in arrays):
        raise ValueError("every set must be [rows, Z] with the same Z")
    dev = arrays[0].device
    cat = arrays[0].contiguous() if len(arrays) == 1 else torch.cat(list(arrays), 0)
    offs = np.zeros(len(arrays) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([int(a.shape[0]) for a in arrays])
    return cat.float(), torch.from_numpy(offs).to(dev), Z


def latent_stats(mus: Sequence[torch.Tensor]):
    """nm_latent_stats over several cohorts in one launch: per cohort the column means and population variances (np.mean /
    np.var, axis 0) of its [N_k, Z] fp32 device array.  Returns (mean, var), device tensors [n_sets, Z]; an empty cohort's
    rows are NaN."""
    require_gpu(mus[0].device)
    cat, offs, Z = _latent_sets(mus)
    mean = torch.empty(len(mus), Z, dtype=torch.float32, device=cat.device)
    var = torch.empty_like(mean)
    _lib.check(_lib.load().nm_latent_stats(cat.data_ptr(), offs.data_ptr(), len(mus), Z, Z, mean.data_ptr(), var.data_ptr(),
                                           _stream_ptr(cat.device)), "nm_latent_stats")
    return mean, var


def latent_scores(mus: Sequence[torch.Tensor], logvars: Sequence[torch.Tensor], mean: torch.Tensor, var: torch.Tensor):
    """nm_latent_score over several sets in one launch: set k's (mu, logvar) [N_k, Z] against row k of mean / var
    [n_sets, Z].  Returns (zsep, score): per set (mu - mean) / sqrt(var + exp(logvar)) [N_k, Z] and the row mean of its
    absolute values [N_k] (separate_latent_deviation / latent_deviation, utils_vae.py:155-161)."""
    require_gpu(mus[0].device)
    cat_mu, offs, Z = _latent_sets(mus)
    cat_lv, _, Zl = _latent_sets(logvars)
    if Zl != Z or cat_lv.shape != cat_mu.shape or tuple(mean.shape) != (len(mus), Z) or tuple(var.shape) != (len(mus), Z):
        raise ValueError("mu / logvar must have equal shapes per set, mean / var must be [n_sets, Z]")
    mean = mean.to(device=cat_mu.device, dtype=torch.float32).contiguous()
    var = var.to(device=cat_mu.device, dtype=torch.float32).contiguous()
    zsep = torch.empty_like(cat_mu)
    score = torch.empty(cat_mu.shape[0], dtype=torch.float32, device=cat_mu.device)
    _lib.check(_lib.load().nm_latent_score(cat_mu.data_ptr(), cat_lv.data_ptr(), offs.data_ptr(), len(mus), Z, Z, mean.data_ptr(),
                                           var.data_ptr(), zsep.data_ptr(), score.data_ptr(), _stream_ptr(cat_mu.device)),
               "nm_latent_score")
    sizes = [int(m.shape[0]) for m in mus]
    return list(torch.split(zsep, sizes)), list(torch.split(score, sizes))


def adam_step(params: torch.Tensor, grads: torch.Tensor, m: torch.Tensor, v: torch.Tensor, t: int, lr=1e-4,
              betas=(0.9, 0.999), eps=1e-8):
    """Flat Adam on device buffers (nm_adam_step); t is the 1-based step count."""
    lib = _lib.load()
    _lib.check(lib.nm_adam_step(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), params.numel(),
                                lr, betas[0], betas[1], eps, t, _stream_ptr(params.device)), "nm_adam_step")
