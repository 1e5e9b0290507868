"""CPU-side checks of the plain-training pick (NM_F_PLAIN, nm_plain_ok): the symbol is exported, the library is version 11,
the library's truth table on host descriptors, and Job.plain_ok() -- the copy of those conditions the launch path reads off
the jobs -- agrees with the library.  No compute calls: there is no GPU here."""
import ctypes as C

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job, JobSet


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbol_version_and_constants(lib):
    assert "nm_plain_ok" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "nm_plain_ok")
    assert lib.nm_version() == 11
    assert _lib.NM_F_PLAIN == 2048 and _lib.NM_SYNC_ERR_PLAIN == 3
    others = (_lib.NM_F_BACKWARD, _lib.NM_F_ADAM, _lib.NM_F_GRADS, _lib.NM_F_EXPORT, _lib.NM_F_PROFILE, _lib.NM_F_ZGIVEN,
              _lib.NM_F_TRACE, _lib.NM_F_BNSTATS, _lib.NM_F_SPLIT, _lib.NM_F_FAULT_INJECT)
    assert all(_lib.NM_F_PLAIN & f == 0 for f in others)           # a bit of its own
    assert lib.nm_plain_ok(None) == _lib.NM_E_NULL


def _probe(M=3, L=2, Z=10, C_=29, H=(110, 110), D=379):
    """A host descriptor nm_plain_ok accepts (the pattern of tests/test_cabi_cpu.py: _probe)."""
    j = _lib.NmJob()
    j.M, j.L, j.Z, j.C = M, L, Z, C_
    for i, h in enumerate(H):
        j.H[i] = h
    for m in range(min(M, _lib.NM_MAX_MOD)):
        j.mod[m].D = D
        j.mod[m].Kx = (D + C_ + 1 + 31) // 32 * 32
        j.mod[m].x_pitch = (D + 3) // 4 * 4
        j.mod[m].Cz = (C_ + 1 + 7) // 8 * 8
    j.n_rows, j.loss_cap, j.eps_cap = 256, 1, 1
    j.n_params = 118479
    j.wsh = 4096
    j.w_off, j.single_bypass = -1, 1
    return j


def test_plain_ok_truth_table_on_descriptors(lib):
    # what stays a run-time value plays no part: shapes, combiner, bypass, injected eps, shared covariates, the LR table
    for M in (1, 3, 4):
        for combine in _lib.NM_COMBINE.values():
            for bypass in (0, 1):
                ok = _probe(M=M)
                ok.combine, ok.single_bypass = combine, bypass
                assert lib.nm_plain_ok(C.byref(ok)) == 0, (M, combine, bypass)
    ok = _probe(M=3, L=3, Z=8, H=(40, 24, 17), D=70)
    ok.M_enc, ok.eps, ok.shared_cov, ok.lr_table, ok.lr_cap, ok.n_rows = 3, 4096, 1, 4096, 7, 300
    ok.gpart, ok.gpart_stride, ok.grads = 4096, 118528, 4096
    assert lib.nm_plain_ok(C.byref(ok)) == 0
    # every folded feature refuses: 1 = "needs the generic kernel" (not an error status)
    for field, val in (("wide", 1), ("reg_head", 1), ("reg_resid", 4096), ("reg_dres", 4096), ("cls_layers", 2), ("cls_classes", 2),
                       ("dz_extra", 4096), ("out_kind", 1), ("n_private", 2), ("tc_weight", 3e-4), ("w_off", 0), ("M_enc", 2),
                       ("wsh", None), ("out_mu", 4096), ("out_logvar", 4096), ("out_z", 4096), ("M", 0)):
        bad = _probe()
        setattr(bad, field, val)
        assert lib.nm_plain_ok(C.byref(bad)) == 1, field
    for field in ("out_loc", "out_sqerr", "out_rowdev", "dloc_extra", "dloc_rowcoef"):
        for m in range(3):
            bad = _probe()
            setattr(bad.mod[m], field, 4096)
            assert lib.nm_plain_ok(C.byref(bad)) == 1, (field, m)
        beyond = _probe()                                           # (a modality the model does not have is not looked at)
        setattr(beyond.mod[3], field, 4096)
        assert lib.nm_plain_ok(C.byref(beyond)) == 0, field


def _bare_job(spec, tc_weight=0.0, out_loc=False, latent_exports=False, dz_extra=False, rowcoef=False):
    """A Job with the fields plain_ok() reads and no device behind it (Job() itself packs tables on the GPU)."""
    j = object.__new__(Job)
    j.spec = spec
    j.kmods = spec.kernel_modalities()
    nk = len(j.kmods)
    j.tc_weight = tc_weight
    t = torch.zeros(1)
    j.out_mu = j.out_logvar = j.out_z = t if latent_exports else None
    j.out_loc = [t if (out_loc and k == nk - 1) else None for k in range(nk)]
    j.out_sqerr, j.out_rowdev = [None] * nk, [None] * nk
    j.dz_extra = t if dz_extra else None
    j.dloc_extra = [None] * nk
    j.dloc_rowcoef = [t if (rowcoef and k == 0) else None for k in range(nk)]
    return j


def _descriptor(job):
    """The fields of job.struct() that nm_plain_ok reads, filled as Job.struct() and ParamLayout.fill_head fill them."""
    s, d = job.spec, _lib.NmJob()
    d.M, d.M_enc, d.C, d.L, d.Z = len(job.kmods), s.M, s.net_c_dim, len(s.hidden), s.latent
    for i, h in enumerate(s.hidden):
        d.H[i] = h
    d.out_kind = 1 if s.is_dm else 0
    d.n_private = s.n_private
    d.w_off = 0 if s.kind == "weighted_dmvae" else -1
    d.tc_weight = job.tc_weight
    d.wide = int(s.wide)
    d.wsh = 4096
    d.reg_head = 1 if s.kind == "regression" else 0
    if s.kind == "regression":
        d.reg_resid = d.reg_dres = 4096
    d.out_mu = d.out_logvar = d.out_z = 4096 if job.out_mu is not None else None
    d.dz_extra = 4096 if job.dz_extra is not None else None
    for k in range(len(job.kmods)):
        d.mod[k].out_loc = 4096 if job.out_loc[k] is not None else None
        d.mod[k].dloc_rowcoef = 4096 if job.dloc_rowcoef[k] is not None else None
    return d


SE, H2 = [379, 379, 379], [110, 110]


@pytest.mark.parametrize("name,dims,hidden,Z,kind,kw,want", [
    ("SE", SE, H2, 10, "multimodal", {}, True),                                        # the benchmark's model
    ("SM", [379], H2, 10, "multimodal", {}, True),
    ("single", [379], H2, 10, "single", {}, True),                                     # class cVAE
    ("UCA", [379, 379, 379, 1137], H2, 10, "multimodal", {}, True),
    ("small L3", [70, 17, 33], [40, 24, 17], 8, "multimodal", {}, True),
    ("regression", SE, H2, 10, "regression", {}, False),                               # regression head
    ("endtoend", SE, H2, 10, "endtoend", {}, False),                                   # decoder-only modalities
    ("endtoend+hinge", SE, H2, 10, "endtoend", dict(dz_extra=True, rowcoef=True), False),
    ("dmvae", [61, 90, 47], [64, 48], 12, "dmvae", {}, False),                         # private columns, sigmoid output
    ("weighted_dmvae", [61, 90, 47], [64, 48], 12, "weighted_dmvae", {}, False),       # learnable loss weights
    ("mmvaeplus", [61, 90, 47], [64, 48], 12, "mmvaeplus", {}, False),                 # sigmoid output
    ("mvtcae", [61, 90, 47], [64, 48], 12, "mvtcae", dict(tc_weight=3e-4), False),     # total correlation
    ("out_loc", SE, H2, 10, "multimodal", dict(out_loc=True), False),                  # an export buffer set
    ("latent exports", SE, H2, 10, "multimodal", dict(latent_exports=True), False),
    ("dz_extra", SE, H2, 10, "multimodal", dict(dz_extra=True), False),                # a classifier's gradient on z
    ("wide", [61, 90, 47], [300, 300], 12, "multimodal", {}, False),                   # general-shape path
])
def test_job_check_agrees_with_library(lib, name, dims, hidden, Z, kind, kw, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, 3, True, kind)
    job = _bare_job(spec, **kw)
    assert job.plain_ok() == want, name
    assert (lib.nm_plain_ok(C.byref(_descriptor(job))) == 0) == want, name


def test_set_pick_and_switch(monkeypatch):
    """JobSet.plain_pick(): every job must pass; NMHIP_PLAIN=0 switches the kernel off; the verdict follows the jobs'
    descriptor versions."""
    spec = nm.ModelSpec(SE, H2, 10, 3, True, "multimodal")
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec), _bare_job(spec)], False
    js._plain_sig = js._plain_all = None
    for j in js.jobs:
        j._version = 0
    monkeypatch.delenv("NMHIP_PLAIN", raising=False)
    assert js.plain_pick()
    monkeypatch.setenv("NMHIP_PLAIN", "0")
    assert not js.plain_pick()
    monkeypatch.delenv("NMHIP_PLAIN")
    assert js.plain_pick()
    js.jobs[1].out_loc[0] = torch.zeros(1)                          # (enable_exports bumps the version with it)
    js.jobs[1]._version += 1
    assert not js.plain_pick()
    js.jobs[1] = _bare_job(nm.ModelSpec(SE, H2, 10, 3, True, "regression"))
    js.jobs[1]._version = 0
    js._plain_sig = None
    assert not js.plain_pick()
