"""The config-1 loopback flow (tests/test_gpu_loopback.py's: a PS and W = 2 worker processes over
loopback sockets, the switch on the PS GPU) with the workers' packs rounding stochastically
(include/ina_pkt_sr.h).  The PS's parameters after every epoch must equal, bit for bit, the replay of
tests/_sr_pkt_ref.py: worker idx rounds on the stream (seed, step = epoch, sub = idx), the PS applies
local + (float(sum) * 2^-k) * 1/(W+1).  The default rounding still reproduces the oracle's INA update."""
import os
import socket
import sys
import tempfile
import threading

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle as orc
from tests import _sr_pkt_ref as P
from tests.conftest import PKG_ROOT, REPO

pytestmark = pytest.mark.gpu

K, W, EPOCHS, SEED = 16, 2, 3, 0x5EED5EED5EED


def make_small():
    return torch.nn.Linear(100, 1000)                       # 101,000 parameters


def noise(idx, epoch, n):
    g = torch.Generator().manual_seed(1000 * idx + epoch)
    return (torch.randn(n, generator=g) * 1e-2).numpy().astype(np.float32)


def noise_blocks(idx, epoch, n):
    """Updates whose magnitude differs by orders between neighbouring packets."""
    mag = torch.logspace(-7, 1, -(-n // 32)).repeat_interleave(32)[:n].numpy()
    return (noise(idx, epoch, n) * 100 * mag).astype(np.float32)


NOISE = {"flat": noise, "blocks": noise_blocks}


def train_flat(model, idx, epoch, kind="flat"):
    with torch.no_grad():
        v = torch.nn.utils.parameters_to_vector(model.parameters())
        v += torch.from_numpy(NOISE[kind](idx, epoch, v.numel())).to(v.device)
        torch.nn.utils.vector_to_parameters(v, model.parameters())


def train_blocks(model, idx, epoch):
    train_flat(model, idx, epoch, "blocks")


def _worker(idx, port, path, kind, kw):
    for p in (REPO, PKG_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ina_amd.loopback import worker_serve
    worker_serve(idx, W, port, path, make_small, train_blocks if kind == "blocks" else train_flat, **kw)


def run_flow(k, V, kind, **kw):
    """(the initial parameters, the PS's parameters after each epoch)."""
    from ina_amd.loopback import ps_serve
    torch.manual_seed(0)
    model = make_small().cuda()
    local0 = torch.nn.utils.parameters_to_vector(model.parameters()).detach().cpu().numpy()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    seen, errs, listening = [], [], threading.Event()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "switch.sock")
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_worker, args=(i, port, path, kind, kw), daemon=True) for i in range(W)]

        def serve():
            try:
                ps_serve(model, W, EPOCHS, port, path, k=k, V=V, timeout_ms=60000, on_listen=listening.set,
                         on_epoch=lambda e, v, ta, tt: seen.append(v.cpu().numpy().copy()))
            except Exception as e:      # noqa: BLE001 -- reported below
                errs.append(e)
                listening.set()
        th = threading.Thread(target=serve, daemon=True)
        th.start()
        try:
            assert listening.wait(60) and not errs, errs     # the PS listens before a worker connects
            for p in procs:
                p.start()
            th.join(timeout=240)
            for p in procs:
                p.join(timeout=60)
            assert not errs, errs
            assert not th.is_alive()
            assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        finally:
            for p in procs:
                if p.is_alive():
                    p.terminate()
    assert len(seen) == EPOCHS
    return local0, seen


@pytest.mark.timeout(600)
@pytest.mark.parametrize("V", [256, 32])
def test_loopback_with_stochastic_rounding_equals_the_replay(V):
    local, seen = run_flow(K, V, "flat", rounding="stochastic", seed=SEED)
    nearest = local
    for e in range(EPOCHS):
        paras = [(local + noise(i, e, local.size)).astype(np.float32) for i in range(W)]
        qs = [P.quantize(paras[i], K, V, SEED, step=e, sub=i, base=local) for i in range(W)]
        nearest = orc.ps_combine_ina_f32(local, paras, K, 1.0 / (W + 1))
        local = P.ps_update(local, qs, K, V, 1.0 / (W + 1))
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e
    assert not np.array_equal(local, nearest)                # the rounding really differs from to-nearest


@pytest.mark.timeout(600)
def test_loopback_with_stochastic_rounding_and_block_scales_equals_the_replay():
    V = 32
    local, seen = run_flow("block", V, "blocks", rounding="stochastic", seed=SEED)
    for e in range(EPOCHS):
        paras = [(local + noise_blocks(i, e, local.size)).astype(np.float32) for i in range(W)]
        kmin = np.minimum.reduce([P.block_scales([p], V, W, 32, base=local) for p in paras])
        assert kmin.max() - kmin.min() >= 16                 # the packets really carry different scales
        qs = [P.quantize(paras[i], kmin, V, SEED, step=e, sub=i, base=local) for i in range(W)]
        local = P.ps_update(local, qs, kmin, V, 1.0 / (W + 1))
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e


@pytest.mark.timeout(600)
def test_loopback_with_the_default_rounding_is_untouched():
    local, seen = run_flow(K, 32, "flat")
    for e in range(EPOCHS):
        paras = [(local + noise(i, e, local.size)).astype(np.float32) for i in range(W)]
        local = orc.ps_combine_ina_f32(local, paras, K, 1.0 / (W + 1))
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e
