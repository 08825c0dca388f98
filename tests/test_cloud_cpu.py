"""CPU tests of the fused multi-view point-cloud observation (ps_point_cloud,
PandaSim.point_cloud): the new ABI symbols, the workspace arithmetic, and the
pure-Python sampler that tests/test_gpu_cloud.py draws its expected ranks
from, held to the known answers of include/pandasim.h's splitmix64 draw."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ------------------------------------------------------------- the sampler
def draw(seed: int, c: int) -> int:
    """splitmix64 output of counter c under `seed` (mod 2^64)."""
    z = (seed + GOLDEN * (c + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def rank(seed: int, c: int, m: int) -> int:
    """The rank sample counter c takes in a merged cloud of m points: the high
    half of the 128-bit product."""
    return (draw(seed, c) * m) >> 64


def ranks(seed: int, env: int, n_points: int, m: int) -> list:
    """Ranks of env `env`'s n_points samples (c = env * n_points + j)."""
    return [rank(seed, env * n_points + j, m) for j in range(n_points)]


def test_sampler_known_answers():
    assert draw(0, 0) == 0xE220A8397B1DCDAF
    assert rank(0, 0, 1000) == 883
    assert rank(12345, 7, 1000) == 431
    # every rank is inside the cloud, for the smallest and for a huge one
    assert all(rank(s, c, 1) == 0 for s in (0, 1, MASK64) for c in range(50))
    big = (1 << 31) - 1
    assert all(0 <= rank(3, c, big) < big for c in range(1000))
    assert len(set(ranks(0, 0, 257, 1 << 30))) > 250  # a draw, not a constant
    assert ranks(0, 1, 257, 999)[0] == rank(0, 257, 999)


# ----------------------------------------------------------------- the ABI
def test_header_and_signatures_carry_the_new_symbols():
    from pandasim import _lib as L

    src = open(os.path.join(ROOT, "include", "pandasim.h")).read()
    names = set(re.findall(r"\b(ps_[a-z_]+)\s*\(", src))
    lib = L.lib()
    for s in ("ps_cloud_workspace_bytes", "ps_point_cloud"):
        assert s in names and s in L.exported_symbols() and hasattr(lib, s), s
        assert L.SIGNATURES[s][2] == "cloud"
    assert L.CLOUD_SYMBOLS == ("ps_cloud_workspace_bytes", "ps_point_cloud")
    assert "ps_cloud_view" in src and "ps_cloud_crop" in src
    assert lib.ps_abi_version() == int(re.search(r"#define PS_ABI_VERSION (\d+)", src).group(1)) == 6
    import ctypes as C

    assert C.sizeof(L.CloudView) == 16 * 4 * 2 + 16 * 8 and C.sizeof(L.CloudCrop) == 24


def test_workspace_bytes():
    from pandasim import _lib as L

    f = L.lib().ps_cloud_workspace_bytes
    per_tile = 32 + 4 + 4  # validity bits, count, prefix
    assert f(1, 1, 40, 40) == 7 * per_tile  # 1 600 pixels: 6 tiles + a partial one
    assert f(1, 1, 16, 16) == per_tile and f(1, 1, 16, 17) == 2 * per_tile
    base = f(1, 1, 480, 480)
    assert base == 900 * per_tile > 0
    for b in (1, 3, 64, 4096):
        for v in (1, 2, 4, 8):
            assert f(b, v, 480, 480) == b * v * base  # linear in num_envs and n_views
    assert f(1 << 28, 8, 480, 480) == (1 << 28) * 8 * base  # 64-bit arithmetic
    for bad in ((1, 0, 40, 40), (1, 9, 40, 40), (1, 4, 0, 40), (1, 4, 40, 0), (0, 4, 40, 40), (1, -1, 40, 40),
                (1, 1, 4096, 4097),  # 65 552 tiles
                ((1 << 28) + 1, 1, 40, 40)):
        assert f(*bad) == -1, bad
    assert f(1, 1, 4096, 4095) == 65520 * per_tile


def test_grasp_views_are_the_reference_four():
    import pandasim

    assert [v["yaw"] for v in pandasim.GRASP_VIEWS] == [0, 135, 245, 300]
    assert all(v["distance"] == 0.6 and list(v["target_position"]) == [0, 0, 0.1] for v in pandasim.GRASP_VIEWS)
    assert hasattr(pandasim.PandaSim, "point_cloud") and hasattr(pandasim.PandaVecEnv, "point_cloud")
