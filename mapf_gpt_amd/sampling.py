"""Host restatement of the library's action sampler (csrc/gpt.hip: uniform01 + sample_kernel), used
by tests to verify the device sampler and by callers that want reproducible draws off-device.

The reference samples with torch.multinomial (model.py:257) whose stream is device-specific; this
package keys a counter-based RNG by (seed, step, row) instead, so a draw does not depend on batch
chunking or on how instances are sharded over GPUs."""
import numpy as np

_M = (1 << 64) - 1


def uniform01(seed, step, rows):
    """rows: int array of global row ids -> float32 uniforms in [0,1) with 24 random bits."""
    rows = np.asarray(rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64((int(seed) + 0x9E3779B97F4A7C15 * (int(step) + 1)) & _M)
        z = z ^ (rows * np.uint64(0xD1342543DE82EF95))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def sample(logits, seed, step, row0=0, do_sample=True):
    """logits float32 [rows, >=5] -> (actions int32 [rows], margin float32 [rows]); margin = distance of the
    uniform draw to the nearest CDF edge (tests skip rows whose margin is below float round-off)."""
    l = np.asarray(logits, dtype=np.float32)[:, :5]
    best = np.argmax(l, axis=1).astype(np.int32)
    if not do_sample:
        return best, np.full(len(l), np.inf, dtype=np.float32)
    mx = l.max(axis=1, keepdims=True)
    e = np.exp((l - mx).astype(np.float32)).astype(np.float32)
    tot = np.zeros(len(l), dtype=np.float32)
    for i in range(5):
        tot = (tot + e[:, i]).astype(np.float32)
    u = (uniform01(seed, step, np.arange(len(l)) + row0) * tot).astype(np.float32)
    c = np.zeros(len(l), dtype=np.float32)
    act = np.full(len(l), 4, dtype=np.int32)
    done = np.zeros(len(l), dtype=bool)
    margin = np.full(len(l), np.inf, dtype=np.float32)
    for i in range(5):
        c = (c + e[:, i]).astype(np.float32)
        margin = np.minimum(margin, np.abs(u - c) / tot)
        hit = (~done) & (u < c)
        act[hit] = i
        done |= hit
    return act, margin


# ----- training dropout masks (csrc/gpt_kernels_train.h: Drop, drop_hash, drop_keep; model.py:33-34, 59, 66, 71, 82, 88, 129, 175) -----
# A mask is a pure function of (seed, step, site, layer, element index): forward and backward regenerate it, nothing is stored, and it does
# not depend on the precision, the workspace size or the chunking of a call.  Sites: 0 the embedding sum, 1 the attention probabilities,
# 2 attention's residual branch, 3 the MLP's.  Element index: site 1 ((row0 + row) * n_head + head) * 65536 + query * 256 + key, the other
# sites ((row0 + row) * 256 + t) * C + c.  One 64-bit hash serves four consecutive elements, 16 bits each.
DROPOUT_SITES = {"embedding": 0, "attention": 1, "attn_proj": 2, "mlp_proj": 3}


def _fmix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def dropout_threshold(p):
    """p in [0, 1) -> the 16-bit threshold round(p * 65536), at most 65535: an element is kept iff its 16 hash bits are >= it"""
    if not (0.0 <= p < 1.0):
        raise ValueError("dropout p must be in [0, 1)")
    return min(int(np.floor(float(np.float32(p)) * 65536.0 + 0.5)), 65535)      # (p as the C ABI's float takes it)


def dropout_scale(p):
    """the float32 factor 1 / (1 - thr / 65536) of the kept elements"""
    return np.float32(1.0) / np.float32(1.0 - dropout_threshold(p) / 65536.0)


def dropout_key(seed, step, site, layer):
    """the 64-bit key of one mask stream: the sampler's (seed, step) word, the stream id (site, layer) folded in, finalised"""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(step) + 1)) & _M
    z ^= ((int(site) * 256 + int(layer) + 1) * 0xD1342543DE82EF95) & _M
    with np.errstate(over="ignore"):
        return int(_fmix(np.uint64(z)))


def dropout_keep(seed, step, site, layer, index, p):
    """index: int array of element indices -> bool array, True where the element is kept.  Element e takes bits 16 (e & 3) of
    splitmix64(key, e >> 2) = fmix(key + 0x9E3779B97F4A7C15 * ((e >> 2) + 1))."""
    e = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _fmix(np.uint64(dropout_key(seed, step, site, layer)) + np.uint64(0x9E3779B97F4A7C15) * ((e >> np.uint64(2)) + np.uint64(1)))
    bits = (h >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
    return bits >= np.uint64(dropout_threshold(p))
