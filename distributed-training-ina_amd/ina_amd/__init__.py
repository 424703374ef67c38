"""ina_amd -- MI355X-native gradient-aggregation path (drop-in for the in-switch
aggregator and worker quantise/packetise code of distributed-training-INA).

Device ops live in ina_amd.ops (libina.so via ctypes); the reference's host
surfaces are mirrored in ina_amd.communicator (communicator.py), ina_amd.
data_manager (DataManager.py), ina_amd.packet (NGAPacket.py / header_config.py)
and ina_amd.ps (launch.py's aggregate / communication_parallel / Worker); buckets that
outgrow one GPU go through ina_amd.dist (ShardedAggregator: reduce-scatter + all-gather
over RCCL; RangeAggregator: range-split worker slices, one all-gather).  ina_amd.blk holds
the block-scaled ops for any gradient dtype (float32, bfloat16, float16); ina_amd.ef the
quantisers and worker packs with error feedback (a residual carried on the device); ina_amd.wire
the sharded int16 wire's quantisers and decodes for any gradient dtype; ina_amd.sr the quantisers
with unbiased stochastic rounding (counter-based, stateless, any gradient dtype); ina_amd.blk_sr
stochastic rounding together with block scales.
"""
from . import blk, blk_sr, ef, sr, wire  # noqa: F401
from ._lib import (ACT_DROP, ACT_FWD_ACK, ACT_FWD_AGG, ACT_FWD_COLLISION, ACT_FWD_OTHER,  # noqa: F401
                   C128_BYTES, C128_VALUES, FLAG_ACK, FLAG_COLLISION, FLAG_OVERFLOW,
                   FLAG_RESEND, InaError, LIB_PATH, MAX_WORKERS, NGA_HDR_BYTES, NUM_REGISTER)

__version__ = "0.1.0"
