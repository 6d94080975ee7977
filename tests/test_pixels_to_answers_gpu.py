"""From decoded images to answers on the device: ``ResNet101Stage3.forward_pixels`` (resize + normalise in
``pnmn_image_prep``, then the network) against ``forward`` on floats the CPU prepared -- ``preprocess`` of the numpy
restatement of Pillow's resize (tests/helpers/pil_resize_reference.py) -- and ``predict_answers`` on ``"pixels"`` batches
against the same call on ``"image"`` features.  The front end is exact, so every comparison is ``torch.equal``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pil_resize_reference as ref  # noqa: E402

from probnmn.data.feature_extractor import (ResNet101Stage3, extract_features_from_pixels, preprocess)  # noqa: E402

pytestmark = pytest.mark.gpu


def _randomise(model, seed):
    """He-initialised convolutions and batch-norm statistics of a trained network's order of magnitude (as in
    tests/test_feature_extractor.py)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean") or name.endswith(".bias"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            elif t.dim() == 4:
                fan_in = t.size(1) * t.size(2) * t.size(3)
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            else:  # batch-norm weight; small on a block's last norm keeps 30 residual blocks from blowing up
                t.copy_((0.3 if "bn3" in name else 1.0) * (0.75 + 0.5 * torch.rand(t.shape, generator=g)))


@pytest.fixture(scope="module")
def extractor():
    m = ResNet101Stage3()
    _randomise(m, 3)
    return m.to(torch.device("cuda:0"))


def floats_from_the_cpu(pixels: np.ndarray, size) -> torch.Tensor:
    """(N, 3, size[0], size[1]) fp32: what a caller with Pillow hands ``forward``."""
    return preprocess(torch.from_numpy(ref.resize_batch(pixels, size)).permute(0, 3, 1, 2))


def test_forward_pixels_is_forward_on_cpu_prepared_floats(extractor):
    dev = torch.device("cuda:0")
    pixels = np.random.default_rng(5).integers(0, 256, size=(2, 96, 80, 3), dtype=np.uint8)
    want = extractor(floats_from_the_cpu(pixels, (64, 64)).to(dev))
    got = extractor.forward_pixels(torch.from_numpy(pixels).to(dev), size=(64, 64))
    assert got.shape == (2, 1024, 4, 4) and got.is_contiguous(memory_format=torch.channels_last)
    assert float(want.abs().max()) > 0.1 and float((want > 0).float().mean()) > 0.1  # (a dead network compares equal trivially)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        extractor.forward_pixels(torch.from_numpy(pixels).to(dev), size=(64, 48))
    # the extraction loop writes what forward_pixels returns
    out = torch.full((2, 1024, 4, 4), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    batches = [torch.from_numpy(pixels[:1]), torch.from_numpy(pixels[1:])]  # (host batches: the loop moves them)
    assert extract_features_from_pixels(extractor, batches, out, size=(64, 64)) == 2
    assert torch.equal(out, got)


def test_predict_answers_from_pixels(extractor):
    """Four 320x480 images and four questions, two batches: the records of the ``"pixels"`` path are those of ``"image"``
    features that the float path computed from the restatement's resize.  The programs come from the grammar-constrained
    beam search, so every one is valid and every answer is the NMN's on those features."""
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import predict_answers
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64).to(dev)
    questions = synthetic_batch(vocab, 4, seed=21)["question"].to(dev)
    pixels = np.random.default_rng(9).integers(0, 256, size=(4, 320, 480, 3), dtype=np.uint8)
    features = extractor(floats_from_the_cpu(pixels, (224, 224)).to(dev))
    assert features.shape == (4, 1024, 14, 14)
    device_pixels = torch.from_numpy(pixels).to(dev)
    assert torch.equal(extractor.forward_pixels(device_pixels), features)

    cut = (slice(0, 2), slice(2, 4))
    from_pixels = [{"question": questions[s], "pixels": device_pixels[s]} for s in cut]
    from_features = [{"question": questions[s], "image": features[s]} for s in cut]
    kwargs = dict(beam_size=4, constrained=True)
    want = predict_answers(pg, nmn, from_features, vocab, **kwargs)
    got = predict_answers(pg, nmn, from_pixels, vocab, extractor=extractor, **kwargs)
    assert len(want) == 4 and all(r["program_valid"] and r["answer"] != "@@UNKNOWN@@" for r in want)
    assert got == want
    # with "image" present nothing changes, with or without an extractor; without either key, or without an extractor: an error
    assert predict_answers(pg, nmn, from_features, vocab, extractor=extractor, **kwargs) == want
    with pytest.raises(ValueError, match="pixels"):
        predict_answers(pg, nmn, [{"question": questions[:2]}], vocab, extractor=extractor, **kwargs)
    with pytest.raises(ValueError, match="extractor"):
        predict_answers(pg, nmn, from_pixels, vocab, **kwargs)
    assert pg.training and nmn.training
