"""Helpers for tests of the weight-plane cache (csrc/split_body.h, engine.weight_plane_cache).

- Layout: where the planes, inverse row scales and fingerprints of every node-encoder layer sit in the cache buffer (the
  rule of make_cache_layout, csrc/api_internal.h), and the live buffer of a module on the current stream.
- decode_planes: the swizzled fp16 planes [2][K/32][rows][32] back to [2][rows][K].
- A bit-exact numpy mirror of the fingerprint split_rows_body computes for one 8-row chunk:
  finalise(sum over pair positions p of term(p, u_p) mod 2^64), u_p the u64 of two adjacent words of one row.
  `term` is vectorised, so a test can price an edit by the terms it changes instead of hashing the chunk again.
"""
import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1
CHUNK_ROWS = 8
THREADS = 256
PAIRS = 32                     # pairs of words per thread
SLOTS = THREADS * PAIRS        # pair positions per chunk
KEY = 0x9E3779B97F4A7C15       # kFpKey: pair position p has the key p * KEY
SWZ = (0, 2, 3, 1)             # plane_swz(r) = SWZ[(r >> 2) & 3]


def _align(v, a=256):
    return (v + a - 1) // a * a


# -- layout ---------------------------------------------------------------------------------------
def cache_layout(dims):
    """dims: [(K, O)] per node-encoder layer.  Per layer a dict with K, O and the byte offsets of planes (4*O*K bytes), inv
    (4*O) and fp (8*ceil(O/8)), each region starting at a 256-byte boundary; and the total."""
    off, out = 0, []
    for K, O in dims:
        assert K % 8 == 0 and K <= 2048, "(every layer of the models tested has a cache entry)"
        lay = {"K": K, "O": O}
        for name, nbytes in (("planes", 4 * O * K), ("inv", 4 * O), ("fp", 8 * ((O + 7) // 8))):
            lay[name] = off
            off = _align(off + nbytes)
        out.append(lay)
    return out, off


def model_layout(model):
    """cache_layout of a module's node encoder, checked against the library's own mtmc_mpn_weight_cache_bytes."""
    import ctypes
    from mtmc_mpn import _lib, torch_ops
    eng = torch_ops.engine_for(model._config_key)
    dims = [(l.in_dim, l.out_dim) for l in eng.spec.enc_node]
    lays, total = cache_layout(dims)
    assert total == _lib.load().mtmc_mpn_weight_cache_bytes(ctypes.byref(eng.shape_model())), "make_cache_layout changed"
    return lays


def live_cache(model, device=None):
    """The weight-plane cache buffer (uint8) the module's eval forwards on the current stream use (modules.py: the
    engine of the module's configuration, keyed by (device, stream))."""
    import torch
    from mtmc_mpn import torch_ops
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch_ops.engine_for(model._config_key)._wc[(dev, torch.cuda.current_stream(dev).cuda_stream)]


def layer_views(buf, lay):
    """(planes [2][O][K] float64, inv [O] float64, fp [ceil(O/8)] int64) of one layer of the cache buffer."""
    import torch
    K, O = lay["K"], lay["O"]
    planes = decode_planes(buf[lay["planes"]:lay["planes"] + 4 * O * K].view(torch.float16), O, K)
    inv = buf[lay["inv"]:lay["inv"] + 4 * O].view(torch.float32).double()
    fp = buf[lay["fp"]:lay["fp"] + 8 * ((O + 7) // 8)].view(torch.int64)
    return planes, inv, fp


# -- planes ---------------------------------------------------------------------------------------
def decode_planes(planes, rows, K):
    """fp16 planes [2][K/32][rows][32] as the pre-split kernels store them (csrc/gemm_presplit.hip, kPlaneKT note: the eight
    halves k..k+7 of row r sit at ((k/32)*rows + r)*32 + 8*(((k%32)/8) ^ swz(r)), swz(r) = {0, 2, 3, 1}[(r>>2)&3]) ->
    [2][rows][K] float64."""
    import torch
    planes = planes.reshape(2, K // 32, rows, 4, 8)                      # [piece][k-tile][row][stored slot][8]
    r = torch.arange(rows, device=planes.device)
    swz = torch.tensor(SWZ, device=planes.device)[(r >> 2) & 3]
    slot = torch.arange(4, device=planes.device).unsqueeze(0) ^ swz.unsqueeze(1)       # [row][logical slot] -> stored slot
    idx = slot.view(1, 1, rows, 4, 1).expand(2, K // 32, rows, 4, 8)
    logical = torch.gather(planes, 3, idx)                               # [piece][k-tile][row][logical slot][8]
    return logical.permute(0, 2, 1, 3, 4).reshape(2, rows, K).double()


# -- the fingerprint mirror -----------------------------------------------------------------------
def mix64(z):
    """fp_mix (the splitmix64 finaliser), on uint64 arrays."""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def term(p, u):
    """The summand of pair position p (0..SLOTS-1) holding the u64 u (the two words of the pair, low word first)."""
    with np.errstate(over="ignore"):
        return mix64(np.asarray(u, dtype=U64) + np.asarray(p, dtype=U64) * U64(KEY))


def finalise(s):
    """sum (mod 2^64) -> the stored fingerprint; never 0 (a zero-filled cache holds no valid chunk)."""
    s = np.asarray(s, dtype=U64)
    with np.errstate(over="ignore"):
        s = s ^ (s >> U64(29))
        return (s * U64(0xBF58476D1CE4E5B9)) | U64(1)


def _index_map():
    """For every (pair position p, half h): the chunk row and column k of the word, from split_rows_body's thread map:
    thread t = wave*64 + lane, row = wave*2 + (lane>>5), l = lane & 31; word slot i = (j*2+q)*4+tt, k = (j*32+l)*8 + q*4 + tt;
    pair c = i >> 1 (words 2c, 2c+1), p = t*32 + c."""
    t = np.arange(THREADS)[:, None, None]
    c = np.arange(PAIRS)[None, :, None]
    h = np.arange(2)[None, None, :]
    i = 2 * c + h
    j, q, tt = i >> 3, (i >> 2) & 1, i & 3
    lane = t & 63
    row = (t >> 6) * 2 + (lane >> 5)
    k = (j * 32 + (lane & 31)) * 8 + q * 4 + tt
    shape = (THREADS, PAIRS, 2)
    return np.broadcast_to(row, shape).reshape(SLOTS, 2), np.broadcast_to(k, shape).reshape(SLOTS, 2)


PAIR_ROW, PAIR_K = _index_map()                 # [SLOTS][2]: row / column of the low and the high word of each pair
ROW_OF_SLOT = PAIR_ROW[:, 0]


def slot_of(row, k):
    """(pair position, half) of the word at (chunk row, column k): the inverse of the index map."""
    row, k = np.asarray(row), np.asarray(k)
    l, j, q, tt = (k >> 3) & 31, k >> 8, (k >> 2) & 1, k & 3
    t = (row >> 1) * 64 + (row & 1) * 32 + l
    i = (j * 2 + q) * 4 + tt
    return t * PAIRS + (i >> 1), i & 1


def chunk_bits(W, chunk):
    """uint32 [8][2048] of the chunk's rows of the fp32 weights W [O][K] (numpy or torch): words at k >= K are 0; plus the
    number of live rows (rows >= O are dead and contribute nothing)."""
    W = np.ascontiguousarray(np.asarray(W, dtype=np.float32))
    O, K = W.shape
    out = np.zeros((CHUNK_ROWS, 2048), dtype=np.uint32)
    rows = W[chunk * CHUNK_ROWS:(chunk + 1) * CHUNK_ROWS]
    out[:rows.shape[0], :K] = rows.view(np.uint32)
    return out, rows.shape[0]


def pair_values(bits):
    """uint64 [SLOTS]: the value of every pair position of a chunk's words (bits: uint32 [8][2048])."""
    lo = bits[PAIR_ROW[:, 0], PAIR_K[:, 0]].astype(U64)
    hi = bits[PAIR_ROW[:, 1], PAIR_K[:, 1]].astype(U64)
    return lo | (hi << U64(32))


def slot_terms(bits, live_rows=CHUNK_ROWS):
    """term of every pair position, 0 for the pairs of dead rows."""
    t = term(np.arange(SLOTS), pair_values(bits))
    t[ROW_OF_SLOT >= live_rows] = 0
    return t


def chunk_sum(bits, live_rows=CHUNK_ROWS):
    return U64(int(slot_terms(bits, live_rows).sum(dtype=U64)))


def fingerprint(W, chunk):
    """The fingerprint split_rows_body stores for chunk `chunk` (rows 8*chunk ..) of the weights W [O][K]."""
    bits, live = chunk_bits(W, chunk)
    return int(finalise(chunk_sum(bits, live)))


def fingerprints(W):
    """The stored fingerprints of every chunk of W [O][K], as int64 (the dtype the tests read the cache with)."""
    O = np.asarray(W).shape[0]
    return np.array([fingerprint(W, c) for c in range((O + 7) // 8)], dtype=U64).view(np.int64)


# -- round 5's hash, kept only to name the positions it could not tell apart --------------------------
def legacy_multiplier_key(row, k):
    """Round 5 multiplied word slot i of thread t by G*(2i+1) * D*(2t+1): positions with equal (2i+1)(2t+1) shared one
    multiplier, so swapping their words, or +d at one and -d at the other, left the sum unchanged."""
    row, k = np.asarray(row), np.asarray(k)
    l, j, q, tt = (k >> 3) & 31, k >> 8, (k >> 2) & 1, k & 3
    t = (row >> 1) * 64 + (row & 1) * 32 + l
    i = (j * 2 + q) * 4 + tt
    return (2 * i + 1) * (2 * t + 1)
