"""shorthair_amd -- MI355X-native Cauchy Reed-Solomon codec (drop-in for catid/shorthair cauchy_256).

The product is the C-ABI shared library ``libcauchy256.so`` (HIP kernels for gfx950 + host code);
this module is a thin ctypes binding used by the tests and the benchmark. It mirrors the
reference interface (cauchy_256.h: ``cauchy_256_init`` / ``cauchy_256_encode`` /
``cauchy_256_decode`` with the same argument meaning and return codes) and exposes the batched
device-resident API (``include/cauchy_256_batch.h``) on torch tensors.

There is no CPU fallback: if the library is missing this import fails, and without a GPU every
codec call returns -2 (see the library's stderr message).
"""
import ctypes
import os

__all__ = ["lib", "Block", "CAUCHY_256_VERSION", "cauchy_256_init", "cauchy_256_encode",
           "cauchy_256_decode", "encode_batch", "decode_batch", "decode_batch_out",
           "encode_batch_var", "decode_batch_out_var", "frame_batch", "unframe_batch", "unframe_scratch_bytes", "wire_emit_batch",
           "rx_list_batch", "rx_list_capacity", "rx_list_scratch_bytes",
           "rx_group_batch", "rx_group_scratch_bytes",
           "rx_window_batch", "rx_window_scratch_bytes", "RxWindow", "RxWindowStruct",
           "RX_WINDOW_MAX_INFO", "RX_HOLD_ALIGN", "RX_WINDOW_SCAN_TILE", "RX_WINDOW_SCAN_PASS",
           "tx_datagram_batch", "tx_datagram_scratch_bytes", "tx_datagram_capacity", "TxGroupDesc",
           "TX_TILE", "TX_TILE_PASS", "TX_MAX_BLOCK_BYTES", "TX_MAX_DATAGRAM_BYTES",
           "RX_GROUP_TILE", "RX_GROUP_TILE_PASS", "RX_GROUP_SLOT_TILE", "RX_GROUP_SLOT_PASS",
           "UNFRAME_TILE_SLOTS", "UNFRAME_SCAN_PASS", "RX_MAX_PACKETS", "RX_INFO_INTS", "RX_SCAN_TILE", "RX_SCAN_PASS",
           "groups_stats",
           "fill_synthetic", "erasure_pattern", "batch_reserve", "batch_errors", "has_fixed", "path", "default_stream", "sync", "LIB_PATH",
           "EXPORTED_SYMBOLS"]

CAUCHY_256_VERSION = 2
LIB_PATH = os.environ.get("SH_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                         "libcauchy256.so")

# Every function declared in include/*.h.
EXPORTED_SYMBOLS = [
    "_cauchy_256_init", "cauchy_256_encode", "cauchy_256_decode",
    "cauchy_256_batch_init", "cauchy_256_encode_batch", "cauchy_256_decode_batch",
    "cauchy_256_decode_batch_out", "cauchy_256_encode_batch_var", "cauchy_256_decode_batch_out_var",
    "cauchy_256_batch_reserve", "cauchy_256_batch_reserve_stream",
    "cauchy_256_batch_errors", "cauchy_256_batch_path", "cauchy_256_fill_synthetic",
    "cauchy_256_erasure_pattern",
    "cauchy_256_default_stream", "cauchy_256_sync", "cauchy_256_profile", "cauchy_256_profile_read",
    "gf256_init_", "gf256_add_mem", "gf256_add2_mem", "gf256_addset_mem", "gf256_mul_mem",
    "gf256_muladd_mem", "gf256_memswap",
    "shorthair_recovery_packet_bytes", "shorthair_encode_groups", "shorthair_recover_groups",
    "shorthair_groups_stats", "shorthair_groups_set_framing", "shorthair_groups_traffic",
    "shorthair_frame_batch", "shorthair_unframe_scratch_bytes", "shorthair_unframe_batch",
    "shorthair_groups_set_delivery", "shorthair_wire_emit_batch", "shorthair_groups_set_wire",
    "shorthair_rx_list_capacity", "shorthair_rx_list_scratch_bytes", "shorthair_rx_list_batch",
    "shorthair_rx_group_scratch_bytes", "shorthair_rx_group_batch",
    "shorthair_rx_window_scratch_bytes", "shorthair_rx_window_batch",
    "shorthair_tx_datagram_scratch_bytes", "shorthair_tx_datagram_capacity", "shorthair_tx_datagram_batch",
]

# include/shorthair_unframe.h: slots per tile sum, and tile sums the scan workgroup takes per pass
UNFRAME_TILE_SLOTS = 256
UNFRAME_SCAN_PASS = 256
# include/shorthair_rx.h: records per group, ints per d_info entry, groups per lane and per pass of the scan
RX_MAX_PACKETS = 512
RX_INFO_INTS = 8
RX_SCAN_TILE = 16
RX_SCAN_PASS = 4096
# include/shorthair_rx.h: datagrams per tile of rx_group_batch, tiles per pass of its tile scan, slots per lane
# and per pass of its slot scan
RX_GROUP_TILE = 256
RX_GROUP_TILE_PASS = 1024
RX_GROUP_SLOT_TILE = 16
RX_GROUP_SLOT_PASS = 4096
# include/shorthair_rx.h: d_info arrays rx_window_batch takes, the alignment of carried records in the hold
# region, slots per lane and per pass of its scan
RX_WINDOW_MAX_INFO = 4
RX_HOLD_ALIGN = 16
RX_WINDOW_SCAN_TILE = 16
RX_WINDOW_SCAN_PASS = 4096
# include/shorthair_tx.h: datagrams per tile of tx_datagram_batch, tiles per pass of its tile scan, the largest
# recovery block and the largest datagram
TX_TILE = 256
TX_TILE_PASS = 1024
TX_MAX_BLOCK_BYTES = 65544
TX_MAX_DATAGRAM_BYTES = 65550

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} not built: run `python shorthair_amd/build.py` "
                      "(the codec has no CPU fallback)")

# One HIP runtime per process. PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 with
# the same SONAMEs as /opt/rocm's: loaded after torch, the library binds to torch's copies; loaded
# before, the process gets two HSA runtimes and whichever initialises second sees no GPU
# (measured on the box: "No HIP GPUs are available" / our -2). So torch, when present, loads
# first. Callers without torch are unaffected.
try:
    import torch  # noqa: F401
except ImportError:
    pass
lib = ctypes.CDLL(LIB_PATH)


class Block(ctypes.Structure):
    """Reference Block descriptor (cauchy_256.h:52-55)."""
    _fields_ = [("data", ctypes.c_void_p), ("row", ctypes.c_ubyte)]


_c = ctypes
lib._cauchy_256_init.argtypes = [_c.c_int]
lib._cauchy_256_init.restype = _c.c_int
lib.cauchy_256_encode.argtypes = [_c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int]
lib.cauchy_256_encode.restype = _c.c_int
lib.cauchy_256_decode.argtypes = [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int]
lib.cauchy_256_decode.restype = _c.c_int
lib.cauchy_256_batch_init.argtypes = [_c.c_int]
lib.cauchy_256_batch_init.restype = _c.c_int
lib.cauchy_256_encode_batch.argtypes = [_c.c_int] * 4 + [_c.c_void_p] * 3
lib.cauchy_256_encode_batch.restype = _c.c_int
lib.cauchy_256_decode_batch.argtypes = [_c.c_int] * 4 + [_c.c_void_p] * 3
lib.cauchy_256_decode_batch.restype = _c.c_int
lib.cauchy_256_decode_batch_out.argtypes = [_c.c_int] * 4 + [_c.c_void_p] * 6
lib.cauchy_256_decode_batch_out.restype = _c.c_int
lib.cauchy_256_encode_batch_var.argtypes = [_c.c_int] * 4 + [_c.c_void_p, _c.c_int] + [_c.c_void_p] * 3
lib.cauchy_256_encode_batch_var.restype = _c.c_int
lib.cauchy_256_decode_batch_out_var.argtypes = [_c.c_int] * 4 + [_c.c_void_p, _c.c_int] + [_c.c_void_p] * 6
lib.cauchy_256_decode_batch_out_var.restype = _c.c_int
lib.shorthair_frame_batch.argtypes = [_c.c_int, _c.c_int, _c.c_void_p, _c.c_longlong] + [_c.c_void_p] * 5
lib.shorthair_frame_batch.restype = _c.c_int
lib.shorthair_unframe_scratch_bytes.argtypes = [_c.c_int, _c.c_int]
lib.shorthair_unframe_scratch_bytes.restype = _c.c_longlong
lib.shorthair_unframe_batch.argtypes = ([_c.c_int] * 3 + [_c.c_longlong] + [_c.c_void_p] * 3 + [_c.c_longlong] +
                                        [_c.c_void_p] * 4)
lib.shorthair_unframe_batch.restype = _c.c_int
lib.shorthair_wire_emit_batch.argtypes = [_c.c_int] * 4 + [_c.c_void_p, _c.c_int] + [_c.c_void_p] * 3
lib.shorthair_wire_emit_batch.restype = _c.c_int
lib.shorthair_rx_list_capacity.argtypes = [_c.c_int] * 3
lib.shorthair_rx_list_capacity.restype = _c.c_int
lib.shorthair_rx_list_scratch_bytes.argtypes = [_c.c_int] * 2
lib.shorthair_rx_list_scratch_bytes.restype = _c.c_longlong
lib.shorthair_rx_list_batch.argtypes = [_c.c_int] * 6 + [_c.c_void_p] * 4 + [_c.c_longlong] + [_c.c_void_p] * 10
lib.shorthair_rx_list_batch.restype = _c.c_int
lib.shorthair_rx_group_scratch_bytes.argtypes = [_c.c_int] * 2
lib.shorthair_rx_group_scratch_bytes.restype = _c.c_longlong
lib.shorthair_rx_group_batch.argtypes = [_c.c_int] * 3 + [_c.c_void_p] * 3 + [_c.c_longlong] + [_c.c_void_p] * 13
lib.shorthair_rx_group_batch.restype = _c.c_int
lib.shorthair_rx_window_scratch_bytes.argtypes = [_c.c_int] * 2
lib.shorthair_rx_window_scratch_bytes.restype = _c.c_longlong
lib.shorthair_rx_window_batch.argtypes = ([_c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int] + [_c.c_void_p] * 6 +
                                          [_c.c_longlong] * 3 + [_c.c_void_p] * 4)
lib.shorthair_rx_window_batch.restype = _c.c_int
lib.shorthair_tx_datagram_scratch_bytes.argtypes = [_c.c_int]
lib.shorthair_tx_datagram_scratch_bytes.restype = _c.c_longlong
lib.shorthair_tx_datagram_capacity.argtypes = [_c.c_int] * 3
lib.shorthair_tx_datagram_capacity.restype = _c.c_longlong
lib.shorthair_tx_datagram_batch.argtypes = ([_c.c_int] * 4 + [_c.c_void_p] * 2 + [_c.c_int, _c.c_void_p, _c.c_longlong] +
                                            [_c.c_void_p] * 3 + [_c.c_longlong, _c.c_void_p, _c.c_int] +
                                            [_c.c_void_p] * 2 + [_c.c_int] + [_c.c_void_p] * 2 +
                                            [_c.c_int, _c.c_void_p, _c.c_longlong] + [_c.c_void_p] * 6)
lib.shorthair_tx_datagram_batch.restype = _c.c_int
lib.shorthair_groups_stats.argtypes = [_c.c_void_p, _c.c_void_p]
lib.shorthair_groups_stats.restype = _c.c_int
lib.cauchy_256_batch_reserve.argtypes = [_c.c_int] * 4
lib.cauchy_256_batch_reserve.restype = _c.c_int
lib.cauchy_256_batch_reserve_stream.argtypes = [_c.c_int] * 4 + [_c.c_void_p]
lib.cauchy_256_batch_reserve_stream.restype = _c.c_int
lib.cauchy_256_batch_errors.argtypes = [_c.c_void_p]
lib.cauchy_256_batch_errors.restype = _c.c_int
lib.cauchy_256_batch_path.argtypes = [_c.c_int] * 3
lib.cauchy_256_batch_path.restype = _c.c_int
lib.cauchy_256_fill_synthetic.argtypes = [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_ulonglong, _c.c_ulonglong, _c.c_void_p]
lib.cauchy_256_fill_synthetic.restype = _c.c_int
lib.cauchy_256_erasure_pattern.argtypes = [_c.c_ulonglong, _c.c_int, _c.c_int, _c.c_ulonglong, _c.c_int,
                                           _c.c_void_p]
lib.cauchy_256_erasure_pattern.restype = _c.c_int
lib.cauchy_256_default_stream.argtypes = []
lib.cauchy_256_default_stream.restype = _c.c_void_p
lib.cauchy_256_sync.argtypes = [_c.c_void_p]
lib.cauchy_256_sync.restype = _c.c_int
lib.cauchy_256_profile.argtypes = [_c.c_int]
lib.cauchy_256_profile.restype = _c.c_int
lib.cauchy_256_profile_read.argtypes = [_c.c_void_p]
lib.cauchy_256_profile_read.restype = _c.c_int


class CodecError(RuntimeError):
    pass


def _check(rc, what):
    if rc == -2:
        raise CodecError(f"{what}: GPU/runtime failure (see stderr)")
    return rc


# ---- reference-shaped single-group API (host buffers; numpy arrays or anything with .ctypes) ----

def cauchy_256_init(version=CAUCHY_256_VERSION):
    """_cauchy_256_init: 0 ok, -1 version mismatch (reference cauchy_256.cpp:390-399)."""
    return _check(lib._cauchy_256_init(version), "cauchy_256_init")


def cauchy_256_encode(k, m, data_ptrs, recovery_ptr, block_bytes):
    """data_ptrs: sequence of k integer addresses; recovery_ptr: address of m*block_bytes."""
    arr = (ctypes.c_void_p * max(k, 1))(*[int(p) for p in data_ptrs])
    return _check(lib.cauchy_256_encode(k, m, arr, int(recovery_ptr), block_bytes), "encode")


def cauchy_256_decode(k, m, blocks, block_bytes):
    """blocks: ctypes array of Block (modified in place, like the reference)."""
    return _check(lib.cauchy_256_decode(k, m, blocks, block_bytes), "decode")


# ---- batched device-resident API on torch tensors ----

def _ptr(t):
    return None if t is None else int(t.data_ptr())


def _addr(t):
    """The packet calls' pointer convention: a cuda tensor, an integer device address or None."""
    return t if t is None or isinstance(t, int) else int(t.data_ptr())


def _size(n, what):
    """The result of a host-only size query: the library answers -1 for bad arguments."""
    if n < 0:
        raise ValueError(f"{what}: bad arguments")
    return n


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return stream


def encode_batch(k, m, block_bytes, groups, data, recovery, stream=None):
    """data: uint8 cuda tensor [groups][k][B]; recovery: [groups][m][B]."""
    return _check(lib.cauchy_256_encode_batch(k, m, block_bytes, groups, _ptr(data), _ptr(recovery),
                                              _stream(stream)), "encode_batch")


def decode_batch(k, m, block_bytes, groups, blocks, rows, stream=None):
    """In place on blocks [groups][k][B] and rows [groups][k] (uint8 cuda tensors)."""
    return _check(lib.cauchy_256_decode_batch(k, m, block_bytes, groups, _ptr(blocks), _ptr(rows),
                                              _stream(stream)), "decode_batch")


def decode_batch_out(k, m, block_bytes, groups, blocks, rows, out, out_rows, out_count, stream=None):
    """Read-only blocks/rows; out [groups][min(k,m)][B], out_rows [groups][min(k,m)], out_count int32 [groups]."""
    return _check(lib.cauchy_256_decode_batch_out(k, m, block_bytes, groups, _ptr(blocks), _ptr(rows),
                                                  _ptr(out), _ptr(out_rows), _ptr(out_count),
                                                  _stream(stream)), "decode_batch_out")


def encode_batch_var(kmax, m, block_bytes, groups, first, total_blocks, data, recovery, stream=None):
    """Var-k encode: first int32 cuda tensor [groups + 1] (group g = blocks first[g]..first[g+1]-1),
    data uint8 [total_blocks][B] packed, recovery [groups][m][B]."""
    return _check(lib.cauchy_256_encode_batch_var(kmax, m, block_bytes, groups, _ptr(first), total_blocks,
                                                  _ptr(data), _ptr(recovery), _stream(stream)),
                  "encode_batch_var")


def decode_batch_out_var(kmax, m, block_bytes, groups, first, total_blocks, blocks, rows, out, out_rows,
                         out_count, stream=None):
    """Var-k out-of-place decode: blocks [total_blocks][B] and rows [total_blocks] packed by `first`;
    out [groups][min(kmax,m)][B], out_rows [groups][min(kmax,m)], out_count int32 [groups]."""
    return _check(lib.cauchy_256_decode_batch_out_var(kmax, m, block_bytes, groups, _ptr(first), total_blocks,
                                                      _ptr(blocks), _ptr(rows), _ptr(out), _ptr(out_rows),
                                                      _ptr(out_count), _stream(stream)),
                  "decode_batch_out_var")


def frame_batch(block_bytes, total_blocks, payload, payload_bytes, off, length, raw, blocks, stream=None):
    """Frame payloads into code blocks on the GPU (include/shorthair_frame.h): block j of blocks
    [total_blocks][B] = [len u16 LE][payload[off[j] : off[j] + length[j]]][zeros], or the B bytes at
    off[j] verbatim where raw[j] != 0. payload uint8, off int64 [total_blocks], length int32
    [total_blocks], raw uint8 [total_blocks] or None, blocks uint8 (8-byte aligned): cuda tensors, or
    integer device addresses."""
    return _check(lib.shorthair_frame_batch(block_bytes, total_blocks, _addr(payload), payload_bytes, _addr(off),
                                            _addr(length), _addr(raw), _addr(blocks), _stream(stream)), "frame_batch")


def unframe_scratch_bytes(groups, emax):
    """Bytes of device scratch unframe_batch needs for (groups, emax). Host only; raises ValueError on
    invalid arguments."""
    return _size(lib.shorthair_unframe_scratch_bytes(groups, emax), "unframe_scratch_bytes")


def unframe_batch(block_bytes, groups, emax, group_stride_blocks, out, out_count, payload, payload_capacity,
                  off, length, scratch, stream=None):
    """Unframe recovered blocks on the GPU (include/shorthair_unframe.h): slot s = g * emax + i reads the
    block at out + (g * group_stride_blocks + i) * B; length[s] = its u16 prefix p, -2 (p > B - 2) or -1
    (i >= out_count[g]); off[s] = the exclusive sum of max(length, 0), off[groups * emax] the total;
    block bytes [2, 2 + p) are packed at payload + off[s]. out uint8 (8-byte aligned), out_count int32
    [groups] or None, payload uint8 [payload_capacity], off int64 [groups * emax + 1], length int32
    [groups * emax], scratch uint8 [unframe_scratch_bytes(groups, emax)]: cuda tensors, or integer device
    addresses."""
    return _check(lib.shorthair_unframe_batch(block_bytes, groups, emax, group_stride_blocks, _addr(out),
                                              _addr(out_count), _addr(payload), payload_capacity, _addr(off),
                                              _addr(length), _addr(scratch), _stream(stream)), "unframe_batch")


def wire_emit_batch(k, m, block_bytes, groups, first, total_blocks, recovery, wire, stream=None):
    """Frame recovery blocks as wire packets on the GPU (include/shorthair_wire.h): record g * m + y of
    wire [groups * m][3 + B] = [k_g + y][k_g - 1][m - 1][recovery[g][y]], k_g = k, or first[g + 1] -
    first[g] with first int32 [groups + 1] (k is then kmax; a malformed group's records are zeros).
    recovery uint8 [groups][m][B] (8-byte aligned), wire uint8 at any address: cuda tensors, or integer
    device addresses; first a tensor, an address or None."""
    return _check(lib.shorthair_wire_emit_batch(k, m, block_bytes, groups, _addr(first), total_blocks, _addr(recovery),
                                                _addr(wire), _stream(stream)), "wire_emit_batch")


def rx_list_capacity(groups, packets, kmax):
    """Entries of each list array of rx_list_batch: min(packets, groups * kmax). Host only; raises
    ValueError on invalid arguments."""
    return _size(lib.shorthair_rx_list_capacity(groups, packets, kmax), "rx_list_capacity")


def rx_list_scratch_bytes(groups, packets):
    """Bytes of device scratch rx_list_batch needs for (groups, packets). Host only; raises ValueError
    on invalid arguments."""
    return _size(lib.shorthair_rx_list_scratch_bytes(groups, packets), "rx_list_scratch_bytes")


def rx_list_batch(kmin, kmax, m, block_bytes, groups, packets, pkt_first, pkt_off, pkt_len, ring, ring_bytes,
                  info, first, slot_group, off, length, raw, rows, summary, scratch, stream=None):
    """List received packets on the GPU (include/shorthair_rx.h): group g holds the records "[id][c][body]"
    of pkt_len[p] bytes at ring + pkt_off[p], p in [pkt_first[g], pkt_first[g + 1]). Writes info int32
    [groups][8] (status, k, m, B, n_orig, n_rec, slot, first_rec), the var-k decode's first int32
    [groups + 1], slot_group int32 [groups], frame_batch's off int64 / length int32 / raw uint8 and the
    decode's rows uint8 (each [rx_list_capacity(groups, packets, kmax)]) and summary int32 [8]. pkt_first
    int32 [groups + 1], pkt_off int64 [packets], pkt_len int32 [packets], ring uint8 [ring_bytes], scratch
    uint8 [rx_list_scratch_bytes(groups, packets)] (8-byte aligned): cuda tensors, or integer device
    addresses."""
    return _check(lib.shorthair_rx_list_batch(kmin, kmax, m, block_bytes, groups, packets, _addr(pkt_first),
                                              _addr(pkt_off), _addr(pkt_len), _addr(ring), ring_bytes, _addr(info),
                                              _addr(first), _addr(slot_group), _addr(off), _addr(length), _addr(raw),
                                              _addr(rows), _addr(summary), _addr(scratch), _stream(stream)),
                  "rx_list_batch")


def rx_group_scratch_bytes(datagrams, groups):
    """Bytes of device scratch rx_group_batch needs for (datagrams, groups). Host only; raises ValueError
    on invalid arguments."""
    return _size(lib.shorthair_rx_group_scratch_bytes(datagrams, groups), "rx_group_scratch_bytes")


def rx_group_batch(datagrams, groups, back, dg_off, dg_len, ring, ring_bytes, state_in, state_out, dg_class, dg_slot,
                   pkt_first, pkt_off, pkt_len, pkt_dg, slot_group, other, summary, scratch, stream=None):
    """Group received datagrams on the GPU (include/shorthair_rx.h): datagram i is the dg_len[i] bytes
    "[seq u16][pong prefix?][g & 0x7f][id][c][body]" at ring + dg_off[i], in arrival order; state_in int32 [1]
    is the unwrapped group number before the batch. Writes state_out int32 [1] (may be state_in), dg_class
    and dg_slot int32 [datagrams], rx_list_batch's pkt_first int32 [groups + 1], pkt_off int64 and pkt_len
    int32 [datagrams], pkt_dg int32 [datagrams], slot_group int32 [groups], other int32 [datagrams] and
    summary int32 [8]. dg_off int64 [datagrams], dg_len int32 [datagrams], ring uint8 [ring_bytes], scratch
    uint8 [rx_group_scratch_bytes(datagrams, groups)] (8-byte aligned): cuda tensors, or integer device
    addresses."""
    return _check(lib.shorthair_rx_group_batch(datagrams, groups, back, _addr(dg_off), _addr(dg_len), _addr(ring), ring_bytes,
                                               _addr(state_in), _addr(state_out), _addr(dg_class), _addr(dg_slot),
                                               _addr(pkt_first), _addr(pkt_off), _addr(pkt_len), _addr(pkt_dg),
                                               _addr(slot_group), _addr(other), _addr(summary), _addr(scratch),
                                               _stream(stream)), "rx_group_batch")


class RxWindowStruct(ctypes.Structure):
    """ShorthairRxWindow (include/shorthair_rx.h): a host struct of device pointers and the capacity."""
    _fields_ = [("base", ctypes.c_void_p), ("first", ctypes.c_void_p), ("off", ctypes.c_void_p),
                ("len", ctypes.c_void_p), ("dg", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("capacity", ctypes.c_int)]


class RxWindow:
    """One of a receiver's two windows on cuda tensors: base int32 [1], first int32 [groups + 1], off int64,
    len and dg int32 [capacity], done uint8 [groups]. first, off and len are rx_list_batch's pkt_first,
    pkt_off and pkt_len with packets = capacity. The tensors are allocated here unless passed in."""

    def __init__(self, groups, capacity, base=None, first=None, off=None, len=None, dg=None, done=None):
        import torch

        def make(t, n, dtype):
            return torch.zeros(n, dtype=dtype, device="cuda") if t is None else t
        self.groups, self.capacity = groups, capacity
        self.base = make(base, 1, torch.int32)
        self.first = make(first, groups + 1, torch.int32)
        self.off = make(off, capacity, torch.int64)
        self.len = make(len, capacity, torch.int32)
        self.dg = make(dg, capacity, torch.int32)
        self.done = make(done, groups, torch.uint8)

    def struct(self):
        return RxWindowStruct(*[int(t.data_ptr()) for t in (self.base, self.first, self.off, self.len, self.dg,
                                                              self.done)], self.capacity)


def rx_window_scratch_bytes(groups, capacity):
    """Bytes of device scratch rx_window_batch needs for (groups, the larger of the two windows' capacities).
    Host only; raises ValueError on invalid arguments."""
    return _size(lib.shorthair_rx_window_scratch_bytes(groups, capacity), "rx_window_scratch_bytes")


def rx_window_batch(groups, prev, infos, datagrams, pkt_first, pkt_off, pkt_len, pkt_dg, slot_group, ring, ring_bytes,
                    hold_off, hold_bytes, nxt, summary, scratch, stream=None):
    """Carry open groups from one receive batch to the next on the GPU (include/shorthair_rx.h): prev (an
    RxWindow, an RxWindowStruct or None for a fresh receiver) and infos (the info tensors of the rx_list_batch
    calls that ran over prev, at most RX_WINDOW_MAX_INFO) give the groups that are done; the open ones' records
    are carried into nxt in front of the new records of rx_group_batch's pkt_first, pkt_off, pkt_len, pkt_dg
    and slot_group, and copied to ring + hold_off when hold_bytes > 0. summary int64 [8], scratch uint8
    [rx_window_scratch_bytes(groups, capacity)] (8-byte aligned): cuda tensors, or integer device addresses."""
    def win(w):
        if w is None or isinstance(w, RxWindowStruct):
            return w
        return w.struct()
    p, n = win(prev), win(nxt)
    infos = list(infos or ())
    arr = (ctypes.c_void_p * max(len(infos), 1))(*[_addr(t) for t in infos])
    return _check(lib.shorthair_rx_window_batch(groups, None if p is None else ctypes.addressof(p), len(infos),
                                                ctypes.addressof(arr), datagrams, _addr(pkt_first), _addr(pkt_off),
                                                _addr(pkt_len), _addr(pkt_dg), _addr(slot_group), _addr(ring), ring_bytes,
                                                hold_off, hold_bytes, None if n is None else ctypes.addressof(n),
                                                _addr(summary), _addr(scratch), _stream(stream)), "rx_window_batch")


class TxGroupDesc(ctypes.Structure):
    """ShorthairTxGroupDesc (include/shorthair_tx.h): 16 bytes; as numpy, dtype [("rec_off", "<i8"), ("m", "<i4"),
    ("block_bytes", "<i4")]."""
    _fields_ = [("rec_off", ctypes.c_longlong), ("m", ctypes.c_int), ("block_bytes", ctypes.c_int)]


def tx_datagram_scratch_bytes(datagrams):
    """Bytes of device scratch tx_datagram_batch needs. Host only; raises ValueError on invalid arguments."""
    return _size(lib.shorthair_tx_datagram_scratch_bytes(datagrams), "tx_datagram_scratch_bytes")


def tx_datagram_capacity(datagrams, max_datagram_bytes, align):
    """Ring bytes that always suffice for `datagrams` datagrams of at most max_datagram_bytes placed at
    multiples of align. Host only; raises ValueError on invalid arguments."""
    return _size(lib.shorthair_tx_datagram_capacity(datagrams, max_datagram_bytes, align), "tx_datagram_capacity")


def tx_datagram_batch(datagrams, groups, m, block_bytes, sched, first, total_blocks, payload, payload_bytes, off,
                      length, recovery, recovery_bytes, group, n_pong, pong_at, pong_val, advance, state_in,
                      state_out, align, ring, ring_bytes, dg_off, dg_len, dg_class, summary, scratch, stream=None):
    """Write datagrams in send order on the GPU (include/shorthair_tx.h): entry sched[i] = -1 (a hole),
    g << 9 | x (original x of slot g) or g << 9 | 256 | y (recovery block y of slot g) becomes
    "[seq u16][pong prefix?][g & 0x7f][id][c][body]" at ring + dg_off[i], dg_off the exclusive sum of the lengths
    rounded up to align. sched int32 [datagrams], first int32 [groups + 1], payload uint8 [payload_bytes], off
    int64 and length int32 [total_blocks], recovery uint8 [recovery_bytes] (8-byte aligned) or None, group
    [groups] of TxGroupDesc (16 bytes each) or None, pong_at int32 [n_pong], pong_val uint32 [2 * n_pong],
    state_in and state_out int32 [2] (may be the same), ring uint8 [ring_bytes], dg_off int64 [datagrams + 1],
    dg_len and dg_class int32 [datagrams], summary int32 [8], scratch uint8
    [tx_datagram_scratch_bytes(datagrams)] (8-byte aligned): cuda tensors, or integer device addresses."""
    return _check(lib.shorthair_tx_datagram_batch(datagrams, groups, m, block_bytes, _addr(sched), _addr(first),
                                                  total_blocks, _addr(payload), payload_bytes, _addr(off), _addr(length),
                                                  _addr(recovery), recovery_bytes, _addr(group), n_pong, _addr(pong_at),
                                                  _addr(pong_val), advance, _addr(state_in), _addr(state_out), align,
                                                  _addr(ring), ring_bytes, _addr(dg_off), _addr(dg_len), _addr(dg_class),
                                                  _addr(summary), _addr(scratch), _stream(stream)),
                  "tx_datagram_batch")


def groups_stats():
    """(launches, groups): cumulative batched codec launches and groups coded by the packet-group layer."""
    a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
    lib.shorthair_groups_stats(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def fill_synthetic(out, n, block_bytes, groups, g0, cfg, stream=None):
    return _check(lib.cauchy_256_fill_synthetic(_ptr(out), n, block_bytes, groups, g0, cfg,
                                                _stream(stream)), "fill_synthetic")


def erasure_pattern(g, k, m, cfg, e_fixed=0):
    """Synthetic decoder input rows of group g (host, no GPU): returns (e, rows uint8[k])."""
    import numpy as np
    rows = np.zeros(k, np.uint8)
    e = lib.cauchy_256_erasure_pattern(g, k, m, cfg, e_fixed, rows.ctypes.data)
    if e < 0:
        raise ValueError("erasure_pattern: bad arguments")
    return e, rows


def batch_reserve(k, m, block_bytes, groups):
    return _check(lib.cauchy_256_batch_reserve(k, m, block_bytes, groups), "batch_reserve")


def batch_errors(stream=None):
    """Malformed decode groups since the last call (waits for the stream)."""
    return _check(lib.cauchy_256_batch_errors(_stream(stream)), "batch_errors")


def has_fixed(k, m, block_bytes):
    """True when (k, m, block_bytes) runs on compile-time-scheduled kernels."""
    return lib.cauchy_256_batch_path(k, m, block_bytes) == 1


def path(k, m, block_bytes):
    """Kernel family that codes (k, m, block_bytes): "fixed" (compile-time schedules), "tile"
    (runtime-coefficient snippet tiles), "generic" (per-column kernels, B/8 < 16) or "invalid".
    Host-only: never initialises the GPU."""
    rc = lib.cauchy_256_batch_path(k, m, block_bytes)
    return {1: "fixed", 2: "tile", 0: "generic"}.get(rc, "invalid")


def default_stream():
    return lib.cauchy_256_default_stream()


def sync(stream=None):
    return _check(lib.cauchy_256_sync(stream), "sync")


def profile(capacity=64):
    """Record HIP events around the stages of the next `capacity` batched decodes (0: off;
    negative: only the two events around stage A of the next -capacity decodes)."""
    return _check(lib.cauchy_256_profile(int(capacity)), "profile")


def profile_read():
    """Mean (setup_ms, stageA_ms, stageB_ms) over the recorded decodes, or None."""
    ms = (ctypes.c_float * 3)()
    return tuple(ms) if lib.cauchy_256_profile_read(ms) > 0 else None
