"""CPU-side checks of the two entry points of csrc/nm_fusion.hip (nm_combine_latent, nm_total_correlation): they are
exported and return their argument errors before they touch a device.  No compute calls: no GPU here."""
import pytest

from multi_modal_normative_modeling_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


P = 4096                                                              # (any non-null address: the checks come first)


def _combine(lib, mus=P, variances=P, M=3, n=100, combine=0, alpha=None, bypass=0, in_log=0, out_log=0, floor=0.0, out_mu=P,
             out_var=P):
    return lib.nm_combine_latent(mus, variances, M, n, combine, alpha, bypass, in_log, out_log, floor, out_mu, out_var, None)


def test_symbols_are_exported(lib):
    for sym in ("nm_combine_latent", "nm_total_correlation"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym


def test_combine_latent_argument_errors(lib):
    for missing in ("mus", "variances", "out_mu", "out_var"):
        assert _combine(lib, **{missing: None}) == _lib.NM_E_NULL, missing
    for M in (0, 9, -1):
        assert _combine(lib, M=M) == _lib.NM_E_MODALITIES, M
    for n in (0, -1):
        assert _combine(lib, n=n) == _lib.NM_E_GEOMETRY, n
    for combine in (-1, _lib.NM_COMBINE["mopoe"] + 1, 99):
        assert _combine(lib, combine=combine) == _lib.NM_E_COMBINE, combine
    assert _combine(lib, combine=_lib.NM_COMBINE["gpoe"], alpha=None) == _lib.NM_E_NULL          # gPoE needs its weights
    # 256 elements per block: one element beyond 2^31 - 1 blocks
    assert _combine(lib, M=1, n=256 * (2 ** 31 - 1) + 1) == _lib.NM_E_GEOMETRY
    # the order of the checks: a null pointer is reported ahead of everything else, the expert count ahead of the geometry
    assert _combine(lib, mus=None, M=0, n=0, combine=-1) == _lib.NM_E_NULL
    assert _combine(lib, M=9, n=0, combine=-1) == _lib.NM_E_MODALITIES
    assert _combine(lib, n=0, combine=-1) == _lib.NM_E_GEOMETRY
    assert b"combin" in lib.nm_status_string(_lib.NM_E_COMBINE).lower()


def test_total_correlation_argument_errors(lib):
    assert lib.nm_total_correlation(None, 3, 19, 6, P, None) == _lib.NM_E_NULL
    assert lib.nm_total_correlation(P, 3, 19, 6, None, None) == _lib.NM_E_NULL
    for M in (0, 9):
        assert lib.nm_total_correlation(P, M, 19, 6, P, None) == _lib.NM_E_MODALITIES, M
    for B, Z in ((0, 6), (-1, 6), (19, 0), (19, 129)):
        assert lib.nm_total_correlation(P, 3, B, Z, P, None) == _lib.NM_E_LATENT, (B, Z)
