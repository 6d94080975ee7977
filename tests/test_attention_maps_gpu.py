"""``NeuralModuleNetwork.forward(..., return_attention=True)`` / ``NMNEngine.attention_maps`` on the MI355X against the CPU
oracle walked module by module (tests/helpers/attention_reference.py): the same tokens have a map, the maps agree to the
NMN parity test's tolerance (tests/test_nmn_gpu.py: rtol = atol = 1e-4), and asking for them changes no answer."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attention_reference  # noqa: E402

from fixtures import encode_programs  # noqa: E402

pytestmark = pytest.mark.gpu

# every module kind (filter, relate, same, intersect, union, query, comparison), a chain a later `scene` drops, an invalid
# program, placeholders and padding, an empty program
CASES = [
    "query_color unique filter_shape[cube] relate[left] unique filter_color[red] scene",
    "count intersect filter_color[red] relate[left] unique filter_shape[cube] scene filter_size[large] relate[right] unique "
    "filter_material[rubber] scene",
    "count union filter_color[red] scene filter_shape[cube] scene",
    "query_shape unique same_color unique filter_size[small] filter_material[metal] scene",
    "equal_color query_color unique filter_shape[cube] scene query_color unique filter_size[large] relate[front] unique "
    "filter_material[metal] scene",
    "greater_than count filter_color[blue] filter_shape[cube] scene count filter_size[small] scene",
    "intersect count scene count scene",
    "count filter_color[red] scene count filter_shape[cube] scene count scene",
    "filter_color[red] query_color scene",
    "@start@ count filter_color[red] scene @end@",
    "exist same_material unique relate[right] unique filter_size[large] scene",
    "",
]
LENGTH = 20


def _setup(size, seed=0):
    from probnmn.models.nmn import NeuralModuleNetwork
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    net = NeuralModuleNetwork(vocab, image_feature_size=(128, size, size), class_projection_channels=128, classifier_linear_size=32)
    programs = encode_programs(CASES, vocab.get_token_to_index_vocabulary("programs"), length=LENGTH)
    g = torch.Generator().manual_seed(seed + 1)
    features = torch.relu(torch.randn(len(CASES), 128, size, size, generator=g))
    answers = torch.randint(0, 28, (len(CASES),), generator=g)
    return vocab, net, programs, features, answers


def _reference(vocab, net, features, programs):
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    return attention_reference.attention_maps(sd, vocab.get_index_to_token_vocabulary("programs"), features, programs)


def _check(out, want_maps, want_mask):
    mask, maps = out["attention_mask"].cpu(), out["attention"].cpu()
    assert mask.dtype == torch.bool and torch.equal(mask, want_mask)
    assert not maps.requires_grad and maps.shape == want_maps.shape
    assert bool((maps[~mask] == 0).all())  # exactly zero where there is no map
    torch.testing.assert_close(maps, want_maps, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("size", [14, 28])
def test_attention_equals_the_oracle_walk_and_changes_nothing(size):
    vocab, net, programs, features, answers = _setup(size)
    want_maps, want_mask = _reference(vocab, net, features, programs)
    assert int(want_mask.sum()) == 28 and float(want_maps[want_mask].std()) > 1e-3
    dev = torch.device("cuda:0")
    net.to(dev).eval()
    f, p, a = features.to(dev), programs.to(dev), answers.to(dev)
    with torch.no_grad():
        plain = net(f, p, a)
        assert "attention" not in plain and "attention_mask" not in plain
        out = net(f, p, a, return_attention=True)
    torch.cuda.synchronize()
    _check(out, want_maps, want_mask)
    assert torch.equal(out["predictions"], plain["predictions"]) and torch.equal(out["loss"], plain["loss"])
    if size == 14:  # with gradients: the maps are detached, the loss and its gradients are those of a plain pass
        net.train()
        net.report_batch_metrics = False
        grads = []
        for flag in (False, True):
            net.zero_grad(set_to_none=True)
            o = net(f, p, a, return_attention=flag)
            o["loss"].mean().backward()
            grads.append((o["loss"].detach().clone(), [q.grad.clone() for q in net.parameters() if q.grad is not None]))
        _check(o, want_maps, want_mask)
        assert torch.equal(grads[0][0], grads[1][0]) and len(grads[0][1]) == len(grads[1][1]) > 0


def test_attention_on_a_trunk_stream_and_of_the_latest_pass():
    vocab, net, programs, features, answers = _setup(14, seed=3)
    want_maps, want_mask = _reference(vocab, net, features, programs)
    dev = torch.device("cuda:0")
    net.to(dev).eval()
    engine = net.engine
    with pytest.raises(RuntimeError):
        engine.attention_maps(LENGTH)  # no forward pass yet
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.no_grad():
        plain = net(features.to(dev), programs.to(dev))
        out = net(features.to(dev), programs.to(dev), trunk_stream=side, return_attention=True)
    torch.cuda.synchronize()
    _check(out, want_maps, want_mask)
    assert torch.equal(out["predictions"], plain["predictions"]) and torch.equal(out["loss"], plain["loss"])

    # a second pass, other programs (the batch reversed) and other features: attention_maps reads THAT pass
    order = torch.arange(len(CASES) - 1, -1, -1)
    features2 = torch.relu(torch.randn(len(CASES), 128, 14, 14, generator=torch.Generator().manual_seed(9)))
    want2, mask2 = _reference(vocab, net, features2, programs[order])
    with torch.no_grad():
        net(features2.to(dev), programs[order].to(dev))
        maps, mask = engine.attention_maps(LENGTH)
    torch.cuda.synchronize()
    _check({"attention": maps, "attention_mask": mask}, want2, mask2)
    with pytest.raises(ValueError):
        engine.attention_maps(LENGTH + 1)
    # the stem of a next pass has started: the arena is about to be rewritten, the old maps are no longer on offer
    with torch.no_grad():
        net.begin(features.to(dev))
    with pytest.raises(RuntimeError):
        engine.attention_maps(LENGTH)
    torch.cuda.synchronize()
