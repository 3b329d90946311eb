"""Table gradients of the rotary paths, the parts that need no GPU: the two new C entries are exported and declared,
vitpe::attention takes the explicit table-gradient flag (default off), and the reference fixture golden/rotary_grad.npz
agrees with the oracle under autograd and with the closed form of the table gradient (cos and sin independent)."""
import os
import re

import numpy as np
import torch

from conftest import rel_err
from oracle import vit_oracle as O

NEW = ("vitpe_apply_rotary_bwd", "vitpe_attention_core_bwd_tables")


def test_new_entries_exported_and_declared():
    from vitpe import _lib
    protos = _lib.parse_header()
    assert len(protos["vitpe_apply_rotary_bwd"]) == 14
    assert len(protos["vitpe_attention_core_bwd_tables"]) == len(protos["vitpe_attention_core_bwd"]) + 3
    out = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    exported = set(re.findall(r"\bT (vitpe_\w+)", out))
    for name in NEW:
        assert name in exported, name
        assert hasattr(_lib.lib(), name)


def test_attention_op_takes_the_table_gradient_flag():
    import vitpe.ops  # noqa: F401
    schema = str(torch.ops.vitpe.attention.default._schema)
    assert schema.endswith("Tensor? cos=None, Tensor? sin=None, bool tables_grad=False) -> (Tensor, Tensor, Tensor)"), schema


def test_fixture_rotary_matches_oracle_and_closed_form(golden):
    """rot/* of the fixture: the oracle's apply_rotary_emb under autograd gives the same gradients, and dcos / dsin are
    sum_(b[, h], q and k) g1 x1 + g2 x2 / g2 x1 - g1 x2 (the formula the kernels implement)."""
    g = golden("rotary_grad")
    CF = O.closed_form_tensor
    q0, k0 = CF("rotary.q", (2, 6, 64, 32)) * 20, CF("rotary.k", (2, 6, 64, 32)) * 20
    dq_up, dk_up = CF("rg.dq", (2, 6, 64, 32)) * 20, CF("rg.dk", (2, 6, 64, 32)) * 20
    for tag, shape in (("shared", (1, 1, 64, 16)), ("per_head", (1, 6, 64, 16))):
        c = (0.8 + CF("rg.cos", shape) * 6).requires_grad_(True)
        s = (CF("rg.sin", shape) * 12).requires_grad_(True)
        q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
        qr, kr = O.apply_rotary_emb(q, k, c, s)
        ((qr * dq_up).sum() + (kr * dk_up).sum()).backward()
        assert rel_err(c.grad, g[f"rot/{tag}/dcos"]) < 1e-6 and rel_err(s.grad, g[f"rot/{tag}/dsin"]) < 1e-6
        assert rel_err(q.grad[:, :, ::8], g[f"rot/{tag}/dq"]) < 1e-6
        dc = ds = 0
        for x, gr in ((q0, dq_up), (k0, dk_up)):
            x1, x2, g1, g2 = x[..., :16], x[..., 16:], gr[..., :16], gr[..., 16:]
            dc = dc + g1 * x1 + g2 * x2
            ds = ds + g2 * x1 - g1 * x2
        red = (0, 1) if tag == "shared" else (0,)
        assert rel_err(dc.sum(red, keepdim=True), g[f"rot/{tag}/dcos"]) < 1e-5
        assert rel_err(ds.sum(red, keepdim=True), g[f"rot/{tag}/dsin"]) < 1e-5
        assert not np.allclose(c.detach() ** 2 + s.detach() ** 2, 1.0)


def test_fixture_is_small(golden):
    from conftest import REPO
    path = os.path.join(REPO, "tests", "golden", "rotary_grad.npz")
    assert os.path.getsize(path) < 500 * 1024
    g = golden("rotary_grad")
    for D in (96, 192):
        for kind in ("angle", "free"):
            for k in ("y", "dx", "dwqkv", "dwproj", "dbproj", "dcos", "dsin"):
                assert f"d{D}/{kind}/{k}" in g.files
