"""Loopback INA training flow with the GPU as the software stand-in for the switch
(BASELINE config 1: worker_num=2, loopback sockets, software stand-in for src/p4).

Control plane exactly as the reference: the PS listens on TCP, pushes the flat
parameter vector to every worker (length-prefixed pickle, worker.py:63-66) and
pulls results back (trans.py:43-54).  Data plane as the INA design intends (and as
the reference never wired together): each worker quantises its update
d_w = p_w - p_global on its GPU, packs NGA-V packets on the GPU and sends them with
sendmmsg to the "switch" socket; the PS runs the P4 state machine
(ngaa.p4:120-196) on its GPU over the received batch (ops.Switch), unpacks the
completed slots, acks them (fragcheck.p4:26-31) and applies
p_global += 1/(W+1) * dequant(sum) -- aggregate()'s update (launch.py:42-52) with
the switch's integer sum in place of the float sum.

The data socket is an AF_UNIX datagram socket by default (loopback, lossless: the
reference has no loss recovery -- its resend bit is unused, headers.p4:33); a UDP
socket on 127.0.0.1 works the same way when the receive buffer is large enough.
"""
from __future__ import annotations

import socket
import time

import torch

from . import _lib, control, ef, ops, ps, sr
from .nic import PacketRing, send_device_packets


class SwitchStandIn:
    """The Tofino's role on the PS GPU for one bucket of n values from W workers."""

    def __init__(self, n: int, W: int, V: int = 256, switch_id: int = 1, device="cuda",
                 num_slots: int | None = None, cp: control.ControlPlane | None = None,
                 ps_addr: str = "127.0.0.1", ps_port: int = 0):
        """cp: the switch's tables (switch_check / ipRoute, ngaa.p4:27-61); by default
        switch_id aggregates and the PS address routes to ps_port.  Only completed
        slots that ipRoute sends to ps_port reach the PS."""
        self.n, self.W, self.V = n, W, V
        if cp is None:
            cp = control.ControlPlane()
            cp.Ingress.switch_check.add_with_set_agg(switch_id)
            cp.Ingress.ipRoute.add_with_ipv4_forward(ps_addr, dst_mac=0, port=ps_port)
        self.cp, self.ps_addr, self.ps_port = cp, control.ip2int(ps_addr), ps_port
        self.npk = -(-n // V)
        # The Tofino pool is 16,384 slots (config.p4:5) and the reference sends a whole
        # bucket with index = seq mod 16384 (DataManager.py:119), so buckets of more
        # packets collide there.  HBM holds a pool for the whole bucket instead.
        self.num_slots = num_slots or max(_lib.NUM_REGISTER, self.npk)
        self.switch = cp.make_switch(V, self.num_slots, device)
        self.ring = PacketRing(W * self.npk, V, device)
        self.out = torch.empty(self.npk * V, dtype=torch.int32, device=device)
        self.acks = torch.zeros((self.npk, self.ring.stride), dtype=torch.uint8, device=device)
        self.device = torch.device(device)

    def _switch_batch(self, sock, timeout_ms):
        want = self.W * self.npk
        got = 0
        while got < want:
            r = self.ring.recv(sock, want - got, timeout_ms, offset=got)
            if r == 0:
                raise TimeoutError(f"switch stand-in: {got}/{want} packets after {timeout_ms} ms")
            got += r
        pk = self.ring.to_device(got)
        act = self.switch.process(pk)
        eg = self.cp.egress(act, dst_default=self.ps_addr)       # ipRoute, ngaa.p4:39-61
        routed = torch.where(eg == self.ps_port, act, torch.zeros_like(act))
        ndone = int((routed == _lib.ACT_FWD_AGG).sum())
        if ndone != self.npk:
            bad = int((act == _lib.ACT_FWD_COLLISION).sum())
            raise RuntimeError(f"{ndone}/{self.npk} slots completed and routed to the PS "
                               f"({bad} collisions)")
        act = routed
        return pk, act

    def aggregate_apply(self, sock, seq0: int, local: torch.Tensor, k, weight_step: float,
                        timeout_ms: int = 30000) -> torch.Tensor:
        """Receive, switch, then ONE fused kernel: completed slots -> dequantise -> update
        (local + weight_step * sum * 2^-k) and PS acks, which then free the slots.  k: the global
        exponent, or an int8 tensor of one exponent per slot (the scales the workers packed with)."""
        pk, act = self._switch_batch(sock, timeout_ms)
        if isinstance(k, torch.Tensor):
            new = ops.apply_completed_blk(pk, act, self.V, seq0, local, k, weight_step, acks=self.acks)
        else:
            new = ops.apply_completed(pk, act, self.V, seq0, local, k, weight_step, acks=self.acks)
        self.switch.process(self.acks)
        return new

    def aggregate(self, sock, seq0: int, timeout_ms: int = 30000) -> torch.Tensor:
        """Receive W x npk packets, run them through the switch, return int32 [n]."""
        pk, act = self._switch_batch(sock, timeout_ms)
        done = torch.nonzero(act == _lib.ACT_FWD_AGG).flatten()
        fin = pk.index_select(0, done)
        fields, vals = ops.unpack_nga(fin, self.V)
        slot = (fields["frag_id"].to(torch.int64) - seq0) % (1 << 32)
        self.out.view(self.npk, self.V).index_copy_(0, slot, vals.view(self.npk, self.V))
        fin[:, 5] = _lib.FLAG_ACK                        # PS ack clears each slot's frag
        self.switch.process(fin)
        return self.out[: self.n]


def _check_rounding(rounding: str, error_feedback: bool):
    if rounding not in ("nearest", "stochastic"):
        raise ValueError(f"unknown rounding {rounding!r}: 'nearest' or 'stochastic'")
    if rounding == "stochastic" and error_feedback:
        raise ValueError("stochastic rounding is the stateless alternative to error feedback: "
                         "rounding='stochastic' is not combined with error_feedback / a residual")


def worker_send(sock, params: torch.Tensor, base: torch.Tensor, worker_id: int, W: int, V: int,
                k, seq0: int, switch_id: int = 1, num_slots: int = _lib.NUM_REGISTER,
                residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                step: int = 0, sub: int = 0) -> int:
    """Worker data plane: quantise(params - base) + NGA-V pack in one GPU pass, then
    sendmmsg.  num_slots must be the aggregator's pool size (index = seq mod num_slots,
    DataManager.py:119).  k: the global exponent, or an int8 tensor of one exponent per packet
    (agree_block_scales).  residual: the worker's error-feedback buffer (ef.new_residual), added
    before the quantiser and updated in place (include/ina_ef.h) -- the EF quantiser, then the
    pack: two launches, in a flow the socket bounds.  rounding="stochastic": the quantiser rounds up
    with the probability of the fraction it would drop (include/ina_pkt_sr.h), from the random stream
    (seed, step, sub), still one launch; not combined with a residual."""
    _check_rounding(rounding, residual is not None)
    if rounding == "stochastic":
        pk = sr.quantize_pack_nga(params.reshape(-1).contiguous(), k, V, bitmap=worker_id, count=W,
                                  switch_id=switch_id, seq0=seq0, seed=seed, step=step, sub=sub,
                                  base=base.reshape(-1).contiguous(), num_slots=num_slots)
        return send_device_packets(sock, pk, _lib.NGA_HDR_BYTES + 4 * V)
    if residual is not None:
        x, b = params.reshape(-1).contiguous(), base.reshape(-1).contiguous()
        if isinstance(k, torch.Tensor):
            q, _ = ef.quantize_blk(x, residual, V, kblk=k, base=b)
        else:
            q = ef.quantize(x, residual, k, base=b)
        pk = ops.pack_nga(q, V, bitmap=worker_id, count=W, switch_id=switch_id, seq0=seq0, num_slots=num_slots)
        return send_device_packets(sock, pk, _lib.NGA_HDR_BYTES + 4 * V)
    pack = ops.quantize_pack_nga_blk if isinstance(k, torch.Tensor) else ops.quantize_pack_nga
    pk = pack(params.reshape(-1).contiguous(), k, V, bitmap=worker_id, count=W,
              switch_id=switch_id, seq0=seq0, base=base.reshape(-1).contiguous(),
              num_slots=num_slots)
    return send_device_packets(sock, pk, _lib.NGA_HDR_BYTES + 4 * V)


def agree_block_scales(conns, mine: torch.Tensor | None = None, device=None) -> torch.Tensor:
    """The per-packet scales of one bucket, agreed over the control connections (ps.send_data
    framing): every worker sends its int8 scales, the PS takes the element-wise MIN (include/ina_blk.h:
    a scale no worker overflows at) and returns it to every worker.
      worker: agree_block_scales(ctl, mine) -- ctl its connection, mine its ops.block_scales(
              [p], V, bits=32, degree=W, base=glob); returns the agreed scales on mine's device.
      PS:     agree_block_scales(conns, device=dev) -- the W connections; returns them on dev."""
    if mine is not None:
        ps.send_data(conns, mine.cpu())
        return ps.get_data(conns).to(mine.device)
    got = [ps.get_data(c) for c in conns]
    for g in got:
        if not isinstance(g, torch.Tensor) or g.dtype != torch.int8 or g.shape != got[0].shape:
            raise ValueError("block scales: every worker sends one int8 tensor of the same length")
    agreed = torch.stack(got).amin(dim=0)
    for c in conns:
        ps.send_data(c, agreed)
    return agreed.to(device) if device is not None else agreed


def seq_base(epoch: int, npk: int) -> int:
    return (1 + epoch * npk) & 0xFFFFFFFF      # send_data numbers from 1 (DataManager.py:106)


def ps_serve(model, W: int, epochs: int, tcp_port: int, data_path: str, k=16,
             V: int = 256, on_epoch=None, timeout_ms: int = 60000, on_listen=None):
    """PS side (master_loop's epoch, launch.py:209-242, with the INA data plane).  k: the global
    exponent of every epoch, or "block": one exponent per packet, agreed with the workers each epoch
    (agree_block_scales) before they pack.  on_listen() is called once both sockets accept peers."""
    if isinstance(k, str) and k != "block":
        raise ValueError(f"unknown k {k!r}: an integer exponent or 'block'")
    dev = next(model.parameters()).device
    local = torch.nn.utils.parameters_to_vector(model.parameters()).detach()
    n = local.numel()
    sw = SwitchStandIn(n, W, V, device=dev)
    data = socket.socket(socket.AF_UNIX, socket.SOCK_DGRAM)
    data.bind(data_path)
    data.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 24)
    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    srv.bind(("127.0.0.1", tcp_port))
    srv.listen(W)
    conns = []
    try:
        if on_listen:
            on_listen()
        for _ in range(W):
            c, _ = srv.accept()
            conns.append(c)
        for c in conns:                                   # init (worker.py:56-61)
            ps.send_data(c, {"para": local.cpu(), "epochs": epochs, "k": k, "V": V,
                             "num_slots": sw.num_slots})
        for epoch in range(epochs):
            t0 = time.time()
            ke = agree_block_scales(conns, device=dev) if k == "block" else k
            new = sw.aggregate_apply(data, seq_base(epoch, sw.npk), local, ke, 1.0 / (W + 1),
                                     timeout_ms)
            t_agg = time.time()
            torch.nn.utils.vector_to_parameters(new, model.parameters())
            local = new
            host = local.cpu()
            for c in conns:                               # push (launch.py:222-227)
                ps.send_data(c, host)
            if on_epoch:
                on_epoch(epoch, local, t_agg - t0, time.time() - t0)
    finally:
        for c in conns:
            c.close()
        srv.close()
        data.close()
    return local


def worker_serve(idx: int, W: int, tcp_port: int, data_path: str, make_model, train_step,
                 device="cuda", error_feedback: bool = False, rounding: str = "nearest", seed: int = 0):
    """Worker side (worker_loop, launch.py:248-322, with the INA data plane).  error_feedback: the
    worker keeps what its quantiser dropped in one residual buffer across the epochs and adds it to
    the next update (include/ina_ef.h); under k = "block" the scales it offers are those of update +
    residual.  rounding="stochastic" (not with error_feedback): the worker's pack rounds stochastically
    (include/ina_pkt_sr.h) under the key `seed`, with the epoch as the step and idx as the stream, so
    workers that share a seed round independently; under k = "block" the scales it offers leave the
    extra quantum (sr.block_scales)."""
    _check_rounding(rounding, error_feedback)
    if rounding == "stochastic":
        sr.check_seed(seed)
    ctl = socket.create_connection(("127.0.0.1", tcp_port))
    data = socket.socket(socket.AF_UNIX, socket.SOCK_DGRAM)
    data.connect(data_path)
    try:
        cfg = ps.get_data(ctl)
        k, V, epochs = cfg["k"], cfg["V"], cfg["epochs"]
        model = make_model().to(device)
        glob = cfg["para"].to(device)
        torch.nn.utils.vector_to_parameters(glob, model.parameters())
        npk = -(-glob.numel() // V)
        resid = ef.new_residual(glob) if error_feedback else None
        for epoch in range(epochs):
            train_step(model, idx, epoch)
            p = torch.nn.utils.parameters_to_vector(model.parameters()).detach()
            ke = k
            if k == "block":
                if rounding == "stochastic":
                    mine = sr.block_scales([p], V, bits=32, degree=W, base=glob)
                else:
                    mine = (ef.block_scales([p], [resid], V, bits=32, degree=W, base=glob) if error_feedback
                            else ops.block_scales([p], V, bits=32, degree=W, base=glob))
                ke = agree_block_scales(ctl, mine)
            worker_send(data, p, glob, idx + 1, W, V, ke, seq_base(epoch, npk),
                        num_slots=cfg["num_slots"], residual=resid, rounding=rounding, seed=seed, step=epoch,
                        sub=idx)
            glob = ps.get_data(ctl).to(device)
            torch.nn.utils.vector_to_parameters(glob, model.parameters())
    finally:
        data.close()
        ctl.close()
