"""LSTM dropout between the encoders' layers, without a GPU: the config keys and constructors accept it (the models carry
p into their nn.LSTM), out-of-range values are refused, and the host reference of the mask (tests/lstm_dropout_ref.py)
has the distribution the contract promises."""
import numpy as np
import pytest

from lstm_dropout_ref import apply, keep_mask, multiplier, scale_of


def test_config_accepts_dropout():
    from probnmn.config import Config

    c = Config(config_override=["PROGRAM_GENERATOR.DROPOUT", 0.2, "QUESTION_RECONSTRUCTOR.DROPOUT", 0.2, "PROGRAM_PRIOR.DROPOUT", 0.1])
    assert c.PROGRAM_GENERATOR.DROPOUT == 0.2 and c.QUESTION_RECONSTRUCTOR.DROPOUT == 0.2 and c.PROGRAM_PRIOR.DROPOUT == 0.1


def _write_vocab(tmp_path):
    from probnmn.vocabulary import Vocabulary

    d = tmp_path / "vocab"
    Vocabulary.clevr().save_to_files(str(d))
    return str(d)


@pytest.mark.parametrize("cls_name", ["ProgramGenerator", "QuestionReconstructor", "ProgramPrior"])
def test_models_carry_dropout(cls_name, tmp_path):
    from probnmn import models
    from probnmn.config import Config
    from probnmn.vocabulary import Vocabulary

    cls = getattr(models, cls_name)
    m = cls(Vocabulary.clevr(), dropout=0.2)
    assert m._encoder._module.dropout == 0.2
    key = {"ProgramGenerator": "PROGRAM_GENERATOR", "QuestionReconstructor": "QUESTION_RECONSTRUCTOR", "ProgramPrior": "PROGRAM_PRIOR"}[cls_name]
    c = Config(config_override=["DATA.VOCABULARY", _write_vocab(tmp_path), key + ".DROPOUT", 0.2])
    assert cls.from_config(c)._encoder._module.dropout == 0.2
    assert getattr(m, "sample_row_offset", None) == 0


@pytest.mark.parametrize("cls_name", ["ProgramGenerator", "QuestionReconstructor", "ProgramPrior"])
def test_out_of_range_dropout_is_refused(cls_name):
    from probnmn import models
    from probnmn.vocabulary import Vocabulary

    with pytest.raises(ValueError):
        getattr(models, cls_name)(Vocabulary.clevr(), dropout=1.5)


def test_mask_extremes():
    assert keep_mask(123, 7, 5, 16, 0.0).all()
    assert not keep_mask(123, 7, 5, 16, 1.0).any()
    x = np.random.default_rng(0).standard_normal((3, 4, 8)).astype(np.float32)
    assert np.array_equal(apply(x, 9, 0.0), x)
    assert not apply(x, 9, 1.0).any()
    assert scale_of(0.2) == np.float32(1.0) / np.float32(0.8)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.8])
def test_keep_rate(p):
    keep = keep_mask(0x1234_5678_9ABC, 256, 16, 256, p, row_offset=1000)  # 2**20 draws
    n = keep.size
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) < 5 * sigma, (keep.mean(), 1 - p)
    m = multiplier(0x1234_5678_9ABC, 4, 3, 8, p)
    assert set(np.unique(m).tolist()) <= {0.0, float(scale_of(p))}


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_rows_steps_and_seeds_are_independent(p):
    """Two rows, two steps or two seeds agree at the rate p**2 + (1 - p)**2 of independent draws."""
    want = p * p + (1 - p) * (1 - p)
    base = keep_mask(77, 512, 8, 256, p)
    pairs = {
        "rows": (base[0::2], base[1::2]),
        "steps": (base[:, 0::2], base[:, 1::2]),
        "seeds": (base, keep_mask(78, 512, 8, 256, p)),
        "row offset": (base[1:], keep_mask(77, 511, 8, 256, p, row_offset=512)),
    }
    for name, (a, b) in pairs.items():
        agree = (a == b).mean()
        sigma = np.sqrt(want * (1 - want) / a.size)
        assert abs(agree - want) < 5 * sigma + 1e-4, (name, agree, want)
    # the row key is row_offset + index: a shifted pass reproduces the same rows' bits
    assert np.array_equal(keep_mask(77, 100, 8, 256, p, row_offset=12), base[12:112])
