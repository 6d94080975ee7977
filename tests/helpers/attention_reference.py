"""Where a program looked, from the CPU oracle: the reference's interpreter loop (``oracle.nmn_oracle.execute_program``,
reference probnmn/models/nmn.py:199-238) walked with the oracle's own module functions, keeping every one-channel output
by the position of the token that produced it -- what ``NeuralModuleNetwork.forward(..., return_attention=True)`` returns.

The interpreter runs every token; the engine runs only the calls the result depends on (a chain whose value a later ``scene``
overwrites before anything reads it is dead).  So each value here carries the positions it was computed from, and a map
counts when the final output depends on it."""
import torch

from oracle import nmn_oracle as oracle


def walk_program(sd, index_to_token, feat_input, program, module_channels):
    """One example (``feat_input`` [1, D, H, W], the stem's output).  Returns ({position: map [H, W]}, valid)."""
    output, saved = (feat_input, frozenset()), None
    maps = {}
    try:
        for p in range(len(program) - 1, -1, -1):
            tok = index_to_token[int(program[p])]
            kind = oracle.module_kind(tok)
            if kind is None:
                continue
            if kind == "scene":
                saved = output
                output = (torch.ones_like(feat_input)[:, :1, :, :], frozenset())
                continue
            if kind == "and":
                value, deps = oracle.and_module(output[0], saved[0]), output[1] | saved[1]
            elif kind == "or":
                value, deps = oracle.or_module(output[0], saved[0]), output[1] | saved[1]
            elif kind == "comparison":
                value, deps = oracle.comparison_module(sd, tok, output[0], saved[0]), output[1] | saved[1]
            else:
                value, deps = oracle._UNARY[kind](sd, tok, feat_input, output[0]), output[1]
            output = (value, deps | {p})
            if value.size(1) == 1:
                maps[p] = value[0, 0]
        if output[0].size(1) != module_channels:
            raise ValueError("program must end with an encoding")
    except Exception:  # (the reference's bare except: an invalid program)
        return {}, 0
    return {p: m for p, m in maps.items() if p in output[1]}, 1


def attention_maps(sd, index_to_token, features, programs):
    """The batch: (maps fp32 [B, T, H, W] with zeros where there is none, mask bool [B, T])."""
    with torch.no_grad():
        feats = oracle.stem(sd, features)
        B, T = programs.shape
        maps = torch.zeros(B, T, feats.size(2), feats.size(3))
        mask = torch.zeros(B, T, dtype=torch.bool)
        for i in range(B):
            found, _ = walk_program(sd, index_to_token, feats[i:i + 1], programs[i].tolist(), feats.size(1))
            for p, m in found.items():
                maps[i, p], mask[i, p] = m, True
    return maps, mask
