"""CPU: the host side of batched sampling -- the per-row seed rule, the per-row sampler list and the argument checks of
generate() for B > 1, which all run before any device work."""
import pytest
import torch
import torch.nn as nn

from gpt4roi_amd.generation import SEED_STRIDE, SamplingConfig, expand_seeds, row_samplers
from gpt4roi_amd.spi_llava import SPILlavaMPTForCausalLM


def test_an_int_seed_expands_by_the_golden_ratio_stride_mod_2_64():
    assert SEED_STRIDE == 0x9E3779B97F4A7C15
    s = 2 ** 64 - 3
    got = expand_seeds(s, 4)
    assert got[0] == s                                       # row 0: the batch-1 stream of the same seed
    assert got == [(s + b * 0x9E3779B97F4A7C15) % 2 ** 64 for b in range(4)]
    assert all(0 <= x < 2 ** 64 for x in got) and len(set(got)) == 4
    assert expand_seeds(7, 1) == [7]


def test_seed_lists_and_drawn_seeds():
    assert expand_seeds([5, 2 ** 64 + 1, -1], 3) == [5, 1, 2 ** 64 - 1]
    with pytest.raises(ValueError):
        expand_seeds([1, 2], 3)
    torch.manual_seed(0)
    a = expand_seeds(None, 5)
    torch.manual_seed(0)
    assert expand_seeds(None, 5) == a and len(a) == 5 and all(0 <= x < 2 ** 62 for x in a)


def test_row_samplers():
    assert row_samplers(None, 3) == [None] * 3
    assert row_samplers((0.2, 50, 1.0), 2) == [(0.2, 50, 1.0)] * 2
    mixed = [(0.2, 50, 1.0), None, (1.0, 5, 0.9)]
    assert row_samplers(mixed, 3) == mixed
    for bad in ([(0.2, 50, 1.0)], [(0.0, 50, 1.0), None], [(1.0, 2000, 1.0), None], [(1.0, 50, 0.0), None],
                [(1.0, 0, 0.5), None]):
        with pytest.raises(ValueError):
            row_samplers(bad, 2)
    with pytest.raises(ValueError):
        row_samplers((1.0, -1, 1.0), 2)


def _bare_lm():
    """The generate() front without a model: argument checks must fail before the model is touched."""
    lm = SPILlavaMPTForCausalLM.__new__(SPILlavaMPTForCausalLM)
    nn.Module.__init__(lm)
    lm.config = type("Cfg", (), {})()
    lm.generation_config = SamplingConfig()
    return lm


@pytest.mark.parametrize("kw,err", [(dict(top_k=2000), ValueError), (dict(top_k=-1), ValueError),
                                    (dict(top_p=0.0), ValueError), (dict(top_p=1.5), ValueError),
                                    (dict(temperature=0.0), ValueError), (dict(seed=[1, 2, 3]), ValueError),
                                    (dict(top_k=0, top_p=0.5), NotImplementedError)])
def test_batched_generate_validates_its_arguments_first(kw, err):
    lm = _bare_lm()
    ids = torch.zeros((2, 5), dtype=torch.int64)
    args = dict(do_sample=True, temperature=0.2, max_new_tokens=4)
    args.update(kw)
    with pytest.raises(err):
        lm.generate(ids, **args)


def test_batch_1_generate_takes_a_one_element_seed_list_only():
    lm = _bare_lm()
    with pytest.raises(ValueError):
        lm.generate(torch.zeros((1, 5), dtype=torch.int64), do_sample=True, temperature=0.2, seed=[1, 2])
