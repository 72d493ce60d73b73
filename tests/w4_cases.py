"""The calls of the GPTQ 4-bit GPU tests and their inputs, shared by
tests/test_w4_ops_gpu.py (runs them) and tests/test_w4_ref.py (proves on the
CPU that the very same inputs have teeth and that the bound is attainable).

Input families per call:
  exact_sparse  x = +-2^j (j in 0..1) on the structural boundary indices, zero
                elsewhere; uniform nibbles; zeros that differ per (group, row)
                and include stored 0 and stored 15 (z + 1 = 16); power-of-two
                scales 2^-2..2^1 that differ per (group, row); qweight words
                with bit 31 set.
  exact_dense   x = +-1 everywhere, same weights.
  Every term of every sum, in the kernel's own form s * sum(q x) - (z+1) s *
  sum(x) too, is a multiple of 2^-2 and the absolute sums stay below 2^24
  quanta (asserted in test_w4_ref.py), so any f32 summation order is exact and
  the GPU output must equal RNE-to-bf16 of the exact sum bit for bit.
  random        Gaussian x, uniform nibbles and zeros, f16 scales:
                |got - ref| <= 2^-8 A + 2^-40, A = sum |W||x| + |res| (the
                derived bf16-output bound of DESIGN.md §2; the in-register
                dequant is exact, so it applies unchanged).
"""
import zlib

import numpy as np

from tests import w4_ref as wr
from tests.helpers import quantize_bf16

TOL_BF16 = 2.0 ** -8
TOL_F32 = 2.0 ** -16
ABS_EPS = 2.0 ** -40
QUANTUM = 2.0 ** -2          # every exact-family term is a multiple of this
FAMILIES = ("exact_sparse", "exact_dense", "random")
REPEATS = 3


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _q(a):
    return quantize_bf16(np.asarray(a, dtype=np.float32))


def boundary_ks(K, g):
    s = {0, 7, 8, 31, 32, g - 1, g, 4095, 4096, 8191, 8192, 16383, 16384,
         K - 33, K - 32, K - 1}
    return np.array(sorted(k for k in s if 0 <= k < K))


# ---- the shapes -------------------------------------------------------------
# (K, g): one group (K = g) at 32/64/128; both sides of the 4096 edge (one
# half-block row set vs 256 lanes) and of every slab edge 8192/16384, each
# with its + 32 tail; g = K; one K per instantiated KB (1, 2, 4, 8)
GEMV_KG = ((32, 32), (64, 64), (128, 128), (4064, 32), (4096, 128),
           (4096, 4096), (4128, 32), (8192, 128), (8224, 32), (8256, 64),
           (16384, 16384), (16416, 32), (32768, 128))
GEMV_N = (8, 24, 40)         # 1, 3, 5 zero-point words per group; 136 (17
                             # words, 34 blocks) runs at K = 4096 below
GEMV_MODES = ((0, False), (1, False), (1, True))    # (epi, alias)
PRODUCT = (64, 14336, 128)   # a row block of the llama3-8b down projection


def kb_of(K):
    return 1 if K <= 4096 else 2 if K <= 8192 else 4 if K <= 16384 else 8


def rows_of(K):
    """Every rows value the launcher instantiates at this K."""
    return (4,) if kb_of(K) == 8 else (4, 8)


def w4_gemv_cases():
    """(N, K, g, epi, alias, rows, repeats) of every op_gemv_w4 call."""
    out = []
    for i, (K, g) in enumerate(GEMV_KG):
        for rows in rows_of(K):
            for mi, (epi, alias) in enumerate(GEMV_MODES):
                N = GEMV_N[(i + mi + rows // 8) % 3]
                if N * K > 1_200_000:
                    N = 24 if 24 * K <= 1_200_000 else 8
                out.append((N, K, g, epi, alias, rows, 1))
    # repeats: one x / res row per launch, back to back
    out += [(24, 4128, 32, 1, True, 4, REPEATS),
            (40, 4096, 128, 1, False, 8, REPEATS),
            (8, 16416, 32, 0, False, 4, REPEATS)]
    # the (rows, KB) pairs of decode_dispatch(LLAMA3_8B_GPTQ) at policy rows
    N, K, g = PRODUCT
    out += [(N, K, g, 1, True, 0, 1), (136, 4096, 128, 0, False, 0, 1),
            (136, 4096, 128, 1, True, 0, 1)]
    return out


def w4_gateup_cases():
    """(I, K, g, rows) of every op_gemv_gateup_w4 call: rows 4 (the only
    instantiation) at every K, rows 0 = the policy at the llama3-8b K."""
    kg = [(8, 32, 32), (24, 128, 64), (8, 4064, 32), (24, 4096, 128),
          (136, 4096, 128), (8, 4128, 32), (24, 8192, 128), (8, 8224, 32),
          (24, 8256, 64), (8, 16384, 16384), (24, 16384, 128)]
    return [c + (4,) for c in kg] + [(136, 4096, 128, 0)]


def w4_dequant_cases():
    """(N, K, g) of every op_dequant_w4 call."""
    return [(8, 32, 32), (24, 128, 64), (40, 4128, 32), (136, 4096, 128),
            (8, 8192, 8192), (24, 16416, 32), (64, 14336, 128)]


# ---- inputs -----------------------------------------------------------------
def weights(fam, rng, N, K, g, scale_rms=None):
    """Checkpoint-layout tensors of one projection."""
    G = K // g
    q = rng.integers(0, 16, size=(K, N))
    z = rng.integers(0, 16, size=(G, N))
    gi, j = np.meshgrid(np.arange(G), np.arange(N), indexing="ij")
    if fam.startswith("exact"):
        z[(gi + j) % 5 == 0] = 15           # z + 1 = 16 must not wrap
        z[(gi + j) % 5 == 2] = 0
        # (the j // n terms: no period of 8, 32 or 64 rows, so a wrong row
        # offset inside a fused tensor shows)
        s = 2.0 ** ((gi * 2 + j * 3 + j // 8 + j // 32 + j // 64) % 4 - 2)
        q[7::8][:, ::2] |= 8                 # bit 31 of every other word set
    else:
        amp = 0.01 if scale_rms is None else scale_rms
        s = (amp * 2.0 ** rng.uniform(-0.5, 0.5, size=(G, N))).astype(
            np.float16).astype(np.float64)
    return wr.pack_gptq(q, z, s)


def exact_x(fam, rng, K, g):
    if fam == "exact_dense":
        return rng.choice([-1.0, 1.0], size=K).astype(np.float32)
    x = np.zeros(K, dtype=np.float32)
    ks = boundary_ks(K, g)
    x[ks] = rng.choice([-1.0, 1.0], size=ks.size) * 2.0 ** rng.integers(
        0, 2, size=ks.size)
    return x


def gemv_inputs(fam, N, K, g, epi, alias, rows, repeats):
    """dict(t = (qweight, qzeros, scales), x (repeats, K), res (repeats, N) or
    None, exact)."""
    rng = _rng("w4gemv", fam, N, K, g, epi, alias, rows, repeats)
    exact = fam.startswith("exact")
    d = dict(exact=exact, res=None)
    d["t"] = weights(fam, rng, N, K, g)
    if exact:
        d["x"] = np.stack([exact_x(fam, rng, K, g) for _ in range(repeats)])
        if epi == 1:
            d["res"] = rng.integers(-40, 41, size=(repeats, N)).astype(
                np.float32)
    else:
        d["x"] = _q(rng.standard_normal((repeats, K)))
        if epi == 1:
            # residual of the size of the product: neither hides the other
            v = wr.dequant(*d["t"], g) @ d["x"][0].astype(np.float64)
            d["res"] = _q(np.sqrt(np.mean(v * v) + 1e-60) *
                          rng.standard_normal((repeats, N)))
    return d


def gemv_expect(d, g, i=0, mut=None, split=None):
    res = d["res"][i] if d["res"] is not None else None
    return wr.gemv_ref(d["t"], g, d["x"][i], res, mut, split)


def gateup_inputs(fam, I, K, g):
    rng = _rng("w4gateup", fam, I, K, g)
    exact = fam.startswith("exact")
    d = dict(exact=exact)
    # random: gate sums of order 1, so silu is in its curved range (q - z - 1
    # has rms ~6.5 over uniform nibbles and zeros)
    d["t"] = weights(fam, rng, 2 * I, K, g, 1.0 / (6.5 * np.sqrt(K)))
    if exact:
        d["x"] = exact_x(fam, rng, K, g)
        if fam == "exact_dense":
            # keep |g| in silu's curved range: scale the whole row sum down
            d["x"] = (d["x"] * 2.0 ** -6).astype(np.float32)
    else:
        d["x"] = _q(rng.standard_normal(K))
    return d


def gateup_bound(val, g, u, Ag, Au):
    """tests/linear_cases.gateup_bound: 2^-8 |ref| + 2^-16 (1.1 A_g |u| +
    |silu(g)| A_u) + 2^-40."""
    return (TOL_BF16 * np.abs(val) + TOL_F32 * (
        1.1 * Ag * np.abs(u) + np.abs(wr.silu(g)) * Au) + ABS_EPS)


def dequant_inputs(fam, N, K, g):
    rng = _rng("w4dequant", fam, N, K, g)
    return weights(fam, rng, N, K, g)


# ---- the defects that fit a call --------------------------------------------
def _weight_mutants(N, K, g, split):
    G = K // g
    m = ["nibble_reversed", "top_nibble_signed", "plus1_dropped",
         "z16_wrapped", "zero_col_next", "zero_col_prev"]
    if N > 8:
        m += ["zero_word_next"]
    if G > 1:
        m += ["zero_group_next", "zero_group_prev", "scale_group_next",
              "scale_group_prev", "scales_untransposed"]
    if split:
        m += ["qkv_offset"]
    return m


def gemv_split(N):
    """Row at which the second projection of a fused tensor would start."""
    return N // 16 * 8 if N >= 16 else 0


def gemv_mutants(N, K, g, epi):
    m = _weight_mutants(N, K, g, gemv_split(N))
    m += ["slab_dropped", "slab_twice", "tail32_dropped", "row_next",
          "row_prev"]
    if K % wr.slab_of(K):               # lanes past K re-load the tail
        m += ["tail32_twice"]
    if epi == 1:
        m += ["res_skipped", "res_doubled", "res_next", "res_prev"]
    return m


def gateup_mutants(I, K, g):
    m = _weight_mutants(2 * I, K, g, I)
    m += ["slab_dropped", "slab_twice", "tail32_dropped", "row_next",
          "row_prev", "gate_up_swapped"]
    if K % wr.slab_of(K):
        m += ["tail32_twice"]
    return m


def moved(exact, base, mutated, bound):
    """The teeth condition: a bit flips (exact family) or some element moves
    by more than twice the bound the GPU test grants."""
    if exact:
        return bool((wr.bf16_bits(base) != wr.bf16_bits(mutated)).any())
    return bool((np.abs(mutated - base) > 2 * bound).any())


def got_bits(got):
    """bf16 pattern of a GPU output that crossed the boundary as f32."""
    return np.ascontiguousarray(got, dtype=np.float32).view(np.uint32) >> 16
