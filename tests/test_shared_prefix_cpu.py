"""CPU: the host side of shared-prefix batches -- generation.plan_shared_prefix and the argument checks of the three new
generate() keywords (shared_prefix=, num_return_sequences=) and of ConversationBot.batch_inputs(pad_side=), which must
all fail before the model is touched (the `_bare_lm` pattern of tests/test_sampling_batch_cpu.py)."""
import pytest
import torch
import torch.nn as nn

from gpt4roi_amd.generation import SamplingConfig, plan_shared_prefix, right_padded_lengths
from gpt4roi_amd.spi_llava import SPILlavaMPTForCausalLM

BBOX = 900
HEAD = [1, 20, 21, 22, 23, 24]                  # what every prompt starts with
BOX_A, BOX_B = [0.1, 0.2, 0.5, 0.6], [0.3, 0.1, 0.9, 0.7]


def test_plan_is_the_longest_common_prefix_of_all_rows():
    rows = [HEAD + [30, 31, 32], HEAD + [30, 41], HEAD + [30, 31, 52, 53]]
    assert plan_shared_prefix(rows, True, None, BBOX) == len(HEAD) + 1
    assert plan_shared_prefix(rows[:1] + rows[2:], True, None, BBOX) == len(HEAD) + 2
    assert plan_shared_prefix([[1, 2, 3], [4, 2, 3]], True, None, BBOX) == 0


def test_plan_is_zero_when_the_images_differ():
    rows = [HEAD + [30, 31], HEAD + [30, 32]]
    assert plan_shared_prefix(rows, False, None, BBOX) == 0
    assert plan_shared_prefix(rows, True, None, BBOX) == len(HEAD) + 1


def test_plan_is_cut_before_the_first_bbox_whose_box_differs():
    a = HEAD + [BBOX, 30, BBOX, 31, 32]
    b = HEAD + [BBOX, 30, BBOX, 31, 33]
    same = plan_shared_prefix([a, b], True, [[BOX_A, BOX_B], [BOX_A, BOX_B]], BBOX)
    assert same == len(HEAD) + 4
    second = plan_shared_prefix([a, b], True, [[BOX_A, BOX_B], [BOX_A, BOX_A]], BBOX)
    assert second == len(HEAD) + 2                          # just before the second <bbox>
    first = plan_shared_prefix([a, b, a], True, [[BOX_A, BOX_B], [BOX_A, BOX_B], [BOX_B, BOX_B]], BBOX)
    assert first == len(HEAD)                               # any row differing cuts, also the last
    missing = plan_shared_prefix([a, b], True, [[BOX_A, BOX_B], [BOX_A]], BBOX)
    assert missing == len(HEAD) + 2                         # a <bbox> without a box is trusted by nobody
    assert plan_shared_prefix([a, b], True, None, BBOX) == len(HEAD)
    tensors = plan_shared_prefix([a, b], True, [torch.tensor([BOX_A, BOX_B]), torch.tensor([BOX_A, BOX_B])], BBOX)
    assert tensors == same


def test_plan_leaves_every_row_a_position_of_its_own():
    rows = [HEAD + [30, 31], HEAD, HEAD + [30]]
    assert plan_shared_prefix(rows, True, None, BBOX) == len(HEAD) - 1          # min n_b - 1
    assert plan_shared_prefix([HEAD, HEAD], True, None, BBOX) == len(HEAD) - 1
    assert plan_shared_prefix([HEAD, []], True, None, BBOX) == 0


def test_plan_of_a_single_row():
    assert plan_shared_prefix([HEAD], True, None, BBOX) == len(HEAD) - 1
    assert plan_shared_prefix([HEAD], False, None, BBOX) == 0
    assert plan_shared_prefix([[7]], True, None, BBOX) == 0
    assert plan_shared_prefix([], True, None, BBOX) == 0


def test_right_padded_lengths():
    m = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0]])
    assert right_padded_lengths(m, 3, 4) == [3, 4, 1]
    assert right_padded_lengths(None, 2, 5) == [5, 5]
    for bad in ([[0, 1, 1, 1]], [[1, 0, 1, 0]], [[0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            right_padded_lengths(torch.tensor(bad), 1, 4)
    with pytest.raises(ValueError):
        right_padded_lengths(m, 2, 4)


def _bare_lm():
    """The generate() front without a model: argument checks must fail before the model is touched."""
    lm = SPILlavaMPTForCausalLM.__new__(SPILlavaMPTForCausalLM)
    nn.Module.__init__(lm)
    lm.config = type("Cfg", (), {})()
    lm.generation_config = SamplingConfig()
    return lm


IDS2 = torch.tensor([[1, 20, 21, 30, 31], [1, 20, 21, 40, 0]])
RIGHT, LEFT = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]]), torch.tensor([[1, 1, 1, 1, 1], [0, 1, 1, 1, 1]])


@pytest.mark.parametrize("kw", [
    dict(shared_prefix=True, attention_mask=LEFT),                     # left padding
    dict(shared_prefix=2, attention_mask=torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 1, 0]])),     # a hole
    dict(shared_prefix=4, attention_mask=RIGHT),                       # the rows share 3 positions, not 4
    dict(shared_prefix=-1, attention_mask=RIGHT),
    dict(shared_prefix=2.0, attention_mask=RIGHT),
    dict(shared_prefix=True, attention_mask=RIGHT[:, :4]),             # a mask of another shape
    dict(shared_prefix=True, attention_mask=RIGHT, bboxes=[torch.zeros(1, 4)]),      # boxes for one row of two
    dict(shared_prefix=True, attention_mask=RIGHT, num_return_sequences=2, do_sample=True),     # n > 1 with B > 1
], ids=["left-padded", "hole", "beyond-the-plan", "negative", "float", "mask-shape", "boxes", "n-with-batch"])
def test_shared_prefix_generate_validates_its_arguments_first(kw):
    lm = _bare_lm()
    with pytest.raises(ValueError):
        lm.generate(IDS2, max_new_tokens=4, **kw)


@pytest.mark.parametrize("kw", [
    dict(num_return_sequences=3),                                      # greedy: n equal rows, as in HF
    dict(num_return_sequences=3, do_sample=False),
    dict(num_return_sequences=0, do_sample=True),
    dict(num_return_sequences=3, do_sample=True, session=object()),
    dict(num_return_sequences=3, do_sample=True, shared_prefix=2),
    dict(num_return_sequences=3, do_sample=True, seed=[1, 2]),         # 2 seeds for 3 rows
    dict(num_return_sequences=3, do_sample=True, attention_mask=torch.tensor([[1, 1, 1, 1, 0]])),
    dict(shared_prefix=True),                                          # one row has nothing to share with
], ids=["greedy-default", "greedy", "zero", "session", "with-shared-prefix", "seeds", "padded-prompt", "batch-1"])
def test_num_return_sequences_validates_its_arguments_first(kw):
    lm = _bare_lm()
    with pytest.raises(ValueError):
        lm.generate(IDS2[:1], max_new_tokens=4, **kw)


def test_batch_inputs_pads_on_the_side_it_is_asked_for():
    from gpt4roi_amd.serve import ConversationBot
    bot = ConversationBot.__new__(ConversationBot)
    bot.device = "cpu"
    bot.tokenizer = type("Tok", (), {"pad_token_id": 0})()
    rows = {"a": torch.tensor([1, 2, 3, 4]), "b": torch.tensor([5, 6])}
    bot.check_input = lambda text, image, hist: (None, text)
    bot.init_inputs = lambda image, text, hist: (dict(input_ids=rows[text], image=torch.zeros(3, 2, 2), bboxes=None), hist)
    _, order, left = bot.batch_inputs(["a", "b"], [None, None], [[], []])
    assert order == [0, 1]
    assert left["input_ids"].tolist() == [[1, 2, 3, 4], [0, 0, 5, 6]] and left["attention_mask"].tolist() == [[1] * 4, [0, 0, 1, 1]]
    _, _, right = bot.batch_inputs(["a", "b"], [None, None], [[], []], pad_side="right")
    assert right["input_ids"].tolist() == [[1, 2, 3, 4], [5, 6, 0, 0]] and right["attention_mask"].tolist() == [[1] * 4, [1, 1, 0, 0]]
    with pytest.raises(ValueError):
        bot.batch_inputs(["a"], [None], [[]], pad_side="middle")


def test_routing_rule_is_the_measured_table(monkeypatch):
    """kernels.shared_attn_wins against the verdicts of profiles/shared_prefix_ab.txt (H = 32, D = 128): the new kernel only
    where it won beyond the spread of the repeats; other head counts were not measured and stay on the existing kernel."""
    from gpt4roi_amd import kernels as K
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", "rule")
    won = {(4, 600), (4, 1500), (8, 600), (8, 1500), (16, 600), (16, 1500), (32, 256), (32, 600), (32, 1500)}
    for B in (2, 4, 8, 16, 32):
        for P in (64, 256, 600, 1500):
            assert K.shared_attn_wins(B, P, 32, 128) == ((B, P) in won), (B, P)
    assert not K.shared_attn_wins(16, 600, 4, 128) and not K.shared_attn_wins(16, 600, 32, 64)
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", "always")
    assert K.shared_attn_wins(2, 0, 4, 128) and K.shared_attn_wins(3, 70, 4, 64) and not K.shared_attn_wins(3, 70, 4, 32)
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", "never")
    assert not K.shared_attn_wins(16, 600, 32, 128)
