"""Generate tests/golden/nmn_reference_layout.json by instantiating the REAL reference's NeuralModuleNetwork (test
infrastructure; runs only where the reference is present, like oracle/make_golden.py, whose stand-ins it uses).

    python oracle/make_checkpoint_layout.py

What is pinned: the layout a reference checkpoint has (CheckpointManager's "nmn" entry, probnmn/utils/checkpointing.py
:68-105) at the reduced dims of tests/test_checkpoint_compat.py -- every state_dict key with its shape in order, and which
keys are parameters, in ``parameters()`` order (torch.optim.Adam's state is indexed by that position).  No values and no
source: tests/test_checkpoint_compat.py rebuilds a module of exactly this layout to write and read checkpoints."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402

DIMS = dict(class_projection_channels=128, classifier_linear_size=32)


def main():
    mg._install_shims()
    mg._load("probnmn.modules.nmn_modules", "probnmn/modules/nmn_modules.py")
    ref_nmn = mg._load("probnmn.models.nmn", "probnmn/models/nmn.py")
    ref = ref_nmn.NeuralModuleNetwork(mg._Vocab(mg.namespaces()), **DIMS)
    layout = {
        "dims": DIMS,
        "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in ref.state_dict().items()],
        "parameters": [k for k, _ in ref.named_parameters()],
    }
    path = os.path.join(mg.OUT, "nmn_reference_layout.json")
    with open(path, "w") as f:  # (one entry per line)
        f.write('{"dims": %s,\n "state_dict": [\n  %s],\n "parameters": [\n  %s]}\n' % (
            json.dumps(DIMS), ",\n  ".join(json.dumps(e) for e in layout["state_dict"]),
            ",\n  ".join(json.dumps(k) for k in layout["parameters"])))
    print("wrote %s: %d state_dict entries, %d parameters" % (path, len(layout["state_dict"]), len(layout["parameters"])))


if __name__ == "__main__":
    main()
