"""``predict_answers(..., explain=True)`` on the MI355X: the answers are those of ``explain=False``; ``steps`` lists, right
to left, exactly the tokens of the program the NMN ran that have an attention map; each ``overlay`` is the numpy
restatement of the overlay kernel (tests/helpers/overlay_reference.py) applied to that step's ``attention`` and the
question's image.  Configuration: the smallest of tests/test_pixels_to_answers_gpu.py (four 320x480 images, two batches)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import overlay_reference  # noqa: E402

from test_pixels_to_answers_gpu import _randomise  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from probnmn.data.feature_extractor import ResNet101Stage3
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    extractor = ResNet101Stage3()
    _randomise(extractor, 3)
    extractor.to(dev)
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64).to(dev)
    questions = synthetic_batch(vocab, 4, seed=21)["question"].to(dev)
    pixels = np.random.default_rng(9).integers(0, 256, size=(4, 320, 480, 3), dtype=np.uint8)
    device_pixels = torch.from_numpy(pixels).to(dev)
    batches = [{"question": questions[s], "pixels": device_pixels[s]} for s in (slice(0, 2), slice(2, 4))]
    return vocab, pg, nmn, extractor, pixels, batches


def _expected_positions(nmn, vocab, program):
    """Token positions with a map, from the program compiler and the planner's specification (no device): the module
    calls, right to left, whose output is one channel wide and which the result depends on."""
    from probnmn.runtime import program_compiler as pc

    stoi = vocab.get_token_to_index_vocabulary("programs")
    row = [stoi[t] for t in program]
    comp = nmn.engine.compiler
    prog = comp.compile(row)
    if not prog.valid:
        return []
    positions = [p for p in range(len(row) - 1, -1, -1) if comp.kinds[row[p]] not in (pc.SKIP, pc.SCENE)]
    live, todo = set(), [prog.result]
    while todo:
        v = todo.pop()
        if v >= 2 and v not in live:
            live.add(v)
            todo += [prog.calls[v - 2].a, prog.calls[v - 2].b]
    return [positions[k] for k, c in enumerate(prog.calls) if c.out_channels == 1 and k + 2 in live]


def _check_steps(records, nmn, vocab, pixels, strength, lut):
    n_steps = 0
    for i, r in enumerate(records):
        want = _expected_positions(nmn, vocab, r["program"])
        assert [s["position"] for s in r["steps"]] == want
        assert want == sorted(want, reverse=True)  # execution order: right to left
        for s in r["steps"]:
            assert s["token"] == r["program"][s["position"]]
            a = s["attention"]
            assert a.dtype == np.float32 and a.shape == (14, 14) and 0.0 <= a.min() and a.max() <= 1.0 and a.std() > 0
            if pixels is None:
                assert "overlay" not in s
            else:
                want_overlay = overlay_reference.overlay(a[None], [0], pixels[i:i + 1], lut, strength)[0]
                assert s["overlay"].dtype == np.uint8 and np.array_equal(s["overlay"], want_overlay)
            n_steps += 1
    return n_steps


def test_explain_with_constrained_beams_and_overlays(setup):
    from probnmn.evaluators import default_colormap, predict_answers

    vocab, pg, nmn, extractor, pixels, batches = setup
    kwargs = dict(beam_size=4, constrained=True, extractor=extractor)
    plain = predict_answers(pg, nmn, batches, vocab, **kwargs)
    got = predict_answers(pg, nmn, batches, vocab, explain=True, **kwargs)
    assert len(got) == 4 and all(r["program_valid"] for r in got)
    assert [{k: v for k, v in r.items() if k != "steps"} for r in got] == plain  # same answers, programs, ranks
    assert _check_steps(got, nmn, vocab, pixels, 160, default_colormap().numpy()) >= 4
    assert pg.training and nmn.training


def test_explain_with_sampled_programs_a_colormap_and_a_strength(setup):
    from probnmn.evaluators import predict_answers

    vocab, pg, nmn, extractor, pixels, batches = setup
    lut = np.random.default_rng(4).integers(0, 256, size=(256, 3), dtype=np.uint8)
    kwargs = dict(constrained_sampling=True, extractor=extractor)
    torch.manual_seed(5)
    plain = predict_answers(pg, nmn, batches, vocab, **kwargs)
    torch.manual_seed(5)
    got = predict_answers(pg, nmn, batches, vocab, explain=True, overlay_strength=255,
                          colormap=torch.from_numpy(lut).to(torch.device("cuda:0")), **kwargs)
    assert [{k: v for k, v in r.items() if k != "steps"} for r in got] == plain
    assert _check_steps(got, nmn, vocab, pixels, 255, lut) >= 4


def test_explain_without_pixels_has_no_overlays(setup):
    from probnmn.evaluators import predict_answers

    vocab, pg, nmn, extractor, pixels, batches = setup
    from_features = [{"question": b["question"], "image": extractor.forward_pixels(b["pixels"])} for b in batches]
    plain = predict_answers(pg, nmn, from_features, vocab, beam_size=4, constrained=True)
    got = predict_answers(pg, nmn, from_features, vocab, beam_size=4, constrained=True, explain=True)
    assert [r["answer"] for r in got] == [r["answer"] for r in plain]
    assert all("program" in r and "steps" in r for r in got)
    assert _check_steps(got, nmn, vocab, None, 160, None) >= 4
