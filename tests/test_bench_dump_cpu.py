"""CPU: bench.dump_outputs - file names, dtypes, the seeded sample of a large sub-network (the same indices every call) and the size bound."""
import os

import numpy as np
import torch

import bench


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Linear(1500, 1500)                     # 2,251,500 values: sampled
        self.small = torch.nn.BatchNorm1d(7)                        # weights + float running stats, and an int64 counter that is skipped


def _load(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_names_dtypes_and_sample(tmp_path):
    torch.manual_seed(0)
    net = _Net()
    log = {"loss": 1.25, "genLoss": 0.5, "CER": 0}
    bench.dump_outputs(str(tmp_path / "a"), net, log)
    bench.dump_outputs(str(tmp_path / "b"), net, log)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["log_CER.npy", "log_genLoss.npy", "log_loss.npy", "weights_big.npy", "weights_small.npy"]
    assert a["log_loss.npy"].dtype == np.float64 and float(a["log_loss.npy"]) == 1.25
    assert a["weights_big.npy"].dtype == np.float32 and a["weights_big.npy"].shape == (bench.DUMP_SAMPLE,)
    assert a["weights_small.npy"].shape == (7 * 4,)                # weight, bias, running_mean, running_var
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    flat = torch.cat([net.big.weight.detach().reshape(-1), net.big.bias.detach()]).numpy()
    assert np.isin(a["weights_big.npy"], flat).all()               # a sample of the network's own values


def test_dump_outputs_stays_within_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 4 * 1000)     # three sub-networks share 3000 values
    net = torch.nn.Module()
    for k in range(3):
        net.add_module("n%d" % k, torch.nn.Linear(100, 100))
    bench.dump_outputs(str(tmp_path), net, {})
    sizes = {n: np.load(os.path.join(tmp_path, n)).size for n in os.listdir(tmp_path)}
    assert sizes == {"weights_n0.npy": 1000, "weights_n1.npy": 1000, "weights_n2.npy": 1000}
