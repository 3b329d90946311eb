"""train.py at the head counts the attention core gained (head dimensions 24, 48, 96 and 128): accepted up front, while
head dimension 16 stays refused with the supported list read from the library.  Needs the built library, no GPU."""
import sys

import pytest

from conftest import REPO


def _train():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import train as T
    return T


def test_train_py_accepts_the_new_head_counts():
    T = _train()
    for ok in (["--num_heads", "8"], ["--num_heads", "4"], ["--num_heads", "2"], ["--embed_dim", "384", "--num_heads", "3"],
               ["--embed_dim", "96", "--num_heads", "4"], ["--embed_dim", "768", "--num_heads", "16"],
               ["--fp32", "--num_heads", "8"], ["--img_size", "224", "--patch_size", "16", "--num_heads", "2"]):
        T.get_args(ok)


def test_train_py_refuses_head_dim_16_and_lists_the_supported_ones(capsys):
    T = _train()
    with pytest.raises(SystemExit):
        T.get_args(["--num_heads", "12"])
    assert "supported head dimensions 24, 32, 48, 64, 96 and 128" in capsys.readouterr().err
    with pytest.raises(SystemExit):   # fp32 hd 128 at 197 tokens: its two backward tiles do not fit
        T.get_args(["--fp32", "--img_size", "224", "--patch_size", "16", "--embed_dim", "384", "--num_heads", "3"])
    assert "at 197 tokens in fp32: head dimensions 24, 32, 48, 64" in capsys.readouterr().err
