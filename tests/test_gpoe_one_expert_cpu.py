"""gPoE on a one-expert model without an alpha parameter (class cVAE with the bypass off): the descriptor must not send the
kernels looking for alpha at offset -1, the float in front of the parameter buffer.  Job.kernel_combine() describes such a job
as the product of experts it is; every model that has its alpha, or several experts, keeps gPoE.  No device."""
import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job


def _job(kind, dims, combine):
    spec = nm.ModelSpec(list(dims), [31, 15], 15, 16, False, kind)
    j = object.__new__(Job)
    j.spec, j.layout, j.combine = spec, nm.ParamLayout(spec), combine
    return j


def test_one_expert_without_alpha_is_described_as_a_product_of_experts():
    j = _job("single", (420,), "gpoe")
    md = _lib.NmJob().mod[0]
    j.layout.fill_modality(md, 0)
    assert md.alpha == -1                                    # what the kernels would index the parameters with
    assert j.kernel_combine() == "poe"


@pytest.mark.parametrize("kind,dims,combine", [
    ("single", (420,), "poe"), ("single", (420,), "moe"), ("single", (420,), "mopoe"),
    ("multimodal", (70,), "gpoe"), ("regression", (89,), "gpoe"), ("multimodal", (61, 90), "gpoe"), ("mvtcae", (61, 90), "gpoe"),
])
def test_every_other_job_keeps_its_combiner(kind, dims, combine):
    j = _job(kind, dims, combine)
    assert j.kernel_combine() == combine
    if combine == "gpoe":
        md = _lib.NmJob().mod[0]
        j.layout.fill_modality(md, 0)
        assert md.alpha >= 0
