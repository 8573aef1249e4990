"""bench.py --dump-outputs on the host: names, dtype, the size budget and a sample that is the same from run to run."""
import os

import numpy as np
import torch

import bench


def _fake_step():
    g = torch.Generator().manual_seed(7)
    loss = {"total_loss": torch.tensor(1.25), "flow_loss": torch.tensor(0.5)}
    out = {"flow": [[torch.randn(2, 2, 8, 8, generator=g)], [torch.randn(3_000_000, generator=g), torch.randn(4, generator=g)]],
           "occ": [torch.randn(2, 1, 8, 8, generator=g)]}
    return loss, out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_layout_budget_and_sample(tmp_path):
    loss, out = _fake_step()
    sizes = bench.dump_outputs(str(tmp_path / "a"), loss, out)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == sorted(sizes) == ["flow_0_0", "flow_1_0", "flow_1_1", "loss_flow_loss", "loss_total_loss", "occ_0"]
    assert all(v.dtype == np.float32 for v in got.values())
    share = bench.DUMP_BUDGET_BYTES // 4 // len(got)
    # small arrays whole, in their shape; the large one as `share` of its elements, in their order
    np.testing.assert_array_equal(got["flow_0_0"], out["flow"][0][0].numpy())
    assert got["loss_total_loss"].shape == () and float(got["loss_total_loss"]) == 1.25
    big = out["flow"][1][0].numpy()
    assert sizes["flow_1_0"] == big.size and got["flow_1_0"].shape == (share,)
    assert np.isin(got["flow_1_0"], big).all()
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 * 2 ** 20
    # a second run on the same values writes the same files
    bench.dump_outputs(str(tmp_path / "b"), loss, out)
    again = _load(str(tmp_path / "b"))
    for k in got:
        np.testing.assert_array_equal(got[k], again[k])
