"""bench.py's options and --dump-outputs (benchlib/dump.py) on the CPU: the files it writes from chunks that stand in for the device's,
their types, their bound of 64 MB, and the same bytes from the same chunks."""
import os
import subprocess
import sys
import zlib
from types import SimpleNamespace

import numpy as np

from benchlib.dump import MAX_BYTES, dump_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Hip:
    def __init__(self, W, H, seed):
        rng = np.random.default_rng(seed)
        n = (W // 16) * (H // 16)
        self.planes = (rng.integers(0, 256, (H, W), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8),
                       rng.integers(0, 256, (H // 2, W // 2), np.uint8))
        self.res = {"MB_parts": rng.integers(0, 4, n, np.int32), "MB_reference_frame": rng.integers(0, 4, n, np.int32),
                    "MB_vectors": rng.integers(-64, 64, (n, 4, 2), np.int16), "MB_coeffs": rng.integers(-2048, 2048, (n, 25, 16), np.int16),
                    "MB_segment_id": rng.integers(0, 4, n, np.int32), "MB_SSIM": rng.random(n, np.float32)}

    def download_last(self):
        return self.planes

    def download_results(self, recon=True):
        assert not recon
        return self.res


class _Driver:
    def __init__(self, W, H, seed):
        self.hip = _Hip(W, H, seed)

    def resolve(self):
        return False


def _leg(W, H, G):
    return SimpleNamespace(G=G, W=W, H=H, mbs=(W // 16) * (H // 16), drv=[_Driver(W, H, k) for k in range(G)])


def test_dump_outputs_types_bound_and_repeatability(tmp_path):
    leg = _leg(1920, 1088, 50)       # more chunks than are sampled
    names = dump_outputs(leg, str(tmp_path / "a"))
    dump_outputs(leg, str(tmp_path / "b"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / "a" / f"{n}.npy")
    assert total <= MAX_BYTES
    crc = np.load(tmp_path / "a" / "recon_crc32.npy")
    assert crc.shape == (50, 3) and crc[3, 0] == zlib.crc32(leg.drv[3].hip.planes[0].tobytes())
    chunks = np.load(tmp_path / "a" / "chunk_index.npy").astype(int)
    y = np.load(tmp_path / "a" / "recon_y.npy")
    assert len(chunks) == y.shape[0] == 48
    assert set(np.unique(y[0])) <= set(np.unique(leg.drv[chunks[0]].hip.planes[0]).astype(np.float32))


def test_dump_outputs_stays_small_at_4k(tmp_path):
    names = dump_outputs(_leg(3840, 2160, 48), str(tmp_path))
    assert sum(os.path.getsize(tmp_path / f"{n}.npy") for n in names) <= MAX_BYTES


def test_only_bitstream_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--only-bitstream"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr
