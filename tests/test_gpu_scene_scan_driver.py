"""Scene cuts in GOP-parallel coding, at the driver (vp8drv_batch_scan_frame_*, vp8drv_batch_scan_result, include/vp8hip_driver.h): the
key frames of the serial loop with scene detection on are vp8host_scene_plan of the differences a batch scans; the batch that scanned
then codes the planned chunks -- members taking chunks from a queue, each started with force_key -- to the serial loop's bytes, frame
for frame; and the settings a scan would disturb are refused with the batch left usable.  64x48, 30 frames, cuts at 6, 8, 21 and 22."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ERR_STATE = -4
W, H, FRAMES, GOP = 64, 48, 30, 9
CUTS = (6, 8, 21, 22)
CFG = dict(gop_size=GOP, num_partitions=2)


class Video:
    """the synthetic sequence's luma; the chroma stands still between the cuts (at this size the sequence's own chroma moves by more
    than scene_change()'s threshold from frame to frame, and detections less than four frames apart defer each other for ever); behind
    every cut another seed, and U shifted by 45"""

    def __init__(self):
        from vp8oclenc_amd.synth import SynthSequence
        seqs = [SynthSequence(W, H, seed=30 + 7 * k) for k in range(len(CUTS) + 1)]
        self.frames = []
        for t in range(FRAMES):
            k = sum(t >= c for c in CUTS)
            y, (_, u, v) = seqs[k].frame(t)[0], seqs[k].frame(0)
            u = np.clip(u.astype(int) + 45 * (k & 1), 0, 255).astype(np.uint8)
            self.frames.append(tuple(np.ascontiguousarray(p) for p in (y, u, v)))

    def frame(self, t):
        return self.frames[t]


@pytest.fixture(scope="module")
def serial():
    """the serial loop with scene detection on, once: (video, every frame's bytes, which are key frames, scene changes counted)"""
    from vp8oclenc_amd import api
    video = Video()
    drv = api.NativeDriver(W, H, scene_detect=1, **CFG)
    frames = []
    for t in range(FRAMES):
        drv.encode_frame_host(*video.frame(t))
        frames.append(drv.get_frame())
    scenes = drv.stats().scene_changes
    drv.close()
    return video, frames, [not (f[0] & 1) for f in frames], scenes


def make_batch(n, setup=None, **cfg):
    from vp8oclenc_amd import api
    drivers = [api.NativeDriver(W, H, **{**CFG, **cfg}) for _ in range(n)]
    for d in drivers:
        if setup:
            setup(d)
    return drivers, api.NativeBatch(drivers)


def code_chunks(drivers, batch, video, chunks):
    """{frame number: bytes}: the members advance independently, a member whose chunk ends takes the next from the queue and starts it
    with force_key, the others carry on (a member without a chunk sits out)"""
    queue, out = list(chunks), {}
    at = [None] * batch.n      # (next frame, end of the chunk)
    first = [False] * batch.n
    while True:
        for i in range(batch.n):
            first[i] = False
            if (at[i] is None or at[i][0] == at[i][1]) and queue:
                s, n = queue.pop(0)
                at[i], first[i] = (s, s + n), True
            elif at[i] is not None and at[i][0] == at[i][1]:
                at[i] = None
        on = [a is not None for a in at]
        if not any(on):
            return out
        planes = [tuple(p.ctypes.data for p in video.frame(a[0])) if a else None for a in at]
        keys = batch.encode_frame_host(planes, on, force_key=first)
        batch.get_frames_begin(on)
        for i in range(batch.n):
            if on[i]:
                assert keys[i] == first[i], (at[i], keys)
                out[at[i][0]] = drivers[i].get_frame_end()
                at[i] = (at[i][0] + 1, at[i][1])


@pytest.mark.parametrize("n", [3, 1])
def test_scan_plan_and_code_give_the_serial_loops_frames(serial, n):
    from vp8oclenc_amd import api, gop_shard
    video, frames, keys, scenes = serial
    assert keys[0] and sum(keys) > (FRAMES + GOP - 1) // GOP and scenes >= 2      # the cuts moved the schedule
    drivers, batch = make_batch(n)
    ud, vd = gop_shard.scan_differences(batch, video, FRAMES)
    detect = lambda t: ud[t] > 7 or vd[t] > 7 or ud[t] + vd[t] > 10
    assert [t for t in range(1, FRAMES) if detect(t)] == list(CUTS)
    plan, by_scene = api.scene_plan(ud, vd, GOP)
    assert list(plan) == keys and int(by_scene.sum()) == scenes
    for d in drivers:      # the scan coded nothing and counted nothing
        s = d.stats()
        assert (s.frame_number, s.key_frames, s.inter_frames, s.scene_changes) == (0, 0, 0, 0)
    chunks = gop_shard.chunks_from_keys(plan)
    assert len(chunks) > n and len({length for _, length in chunks}) > 1      # drivers are reused, chunks of several lengths
    got = code_chunks(drivers, batch, video, chunks)      # the batch that scanned, not a second one
    assert sorted(got) == list(range(FRAMES))
    for t in range(FRAMES):
        assert got[t] == frames[t], f"frame {t}: {len(got[t])} bytes for {len(frames[t])}"
    batch.close()
    for d in drivers:
        d.close()


def test_the_device_scan_is_the_host_scan(serial):
    from vp8oclenc_amd import api
    video = serial[0]
    dev = [[api.to_device(p) for p in video.frame(t)] for t in (5, 6, 7)]
    ptr = {False: [tuple(p.data_ptr() for p in f) for f in dev], True: [tuple(p.ctypes.data for p in video.frame(t)) for t in (5, 6, 7)]}
    got = {}
    for host in (False, True):
        drivers, batch = make_batch(2)
        for call, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):      # member 0 takes frames 5, 6, 7; member 1 frame 6, sits a call out, frame 5
            batch.scan_frame_device([ptr[host][a], ptr[host][b]], [True, call != 1], host=host)
            got[host, call] = batch.scan_result()
        batch.close()
        for d in drivers:
            d.close()
    for call in range(3):
        assert got[False, call] == got[True, call]
    assert got[True, 0] == [(0, 0), (0, 0)]                          # the members' first frames
    assert got[True, 1][1] is None and got[True, 1][0][0] > 7        # frame 6 against 5: the cut
    assert got[True, 2][0][0] <= 7 and got[True, 2][1] == got[True, 1][0]      # 7 against 6: none; 5 against 6: the cut the other way
    for f in dev:
        for p in f:
            p.free()


@pytest.mark.parametrize("what", ["denoise", "deinterlace adaptive", "analysis", "quality statistics"])
def test_settings_a_scan_would_disturb_are_refused_and_the_batch_stays_usable(serial, what):
    """each keeps a history of the frames taken in, or numbers them: VP8HIP_ERR_STATE, nothing changed -- the batch then codes what a
    batch that was never asked codes"""
    from vp8oclenc_amd import api
    video = serial[0]
    setup = {"denoise": lambda d: d.set_denoise(2), "deinterlace adaptive": lambda d: d.set_deinterlace("adaptive", "top"),
             "analysis": lambda d: d.set_analysis(True), "quality statistics": None}[what]
    cfg = dict(quality_stats=1) if what == "quality statistics" else {}
    planes = lambda t: [tuple(p.ctypes.data for p in video.frame(t + 3 * i)) for i in range(2)]
    got = []
    for asked in (True, False):
        drivers, batch = make_batch(2, setup, **cfg)
        if asked:
            for host in (True, False):      # (refused before a pointer is looked at)
                with pytest.raises(api.Vp8HipError) as e:
                    batch.scan_frame_device(planes(0), host=host)
                assert e.value.args[1] == ERR_STATE
            with pytest.raises(api.Vp8HipError):
                batch.scan_result()      # nothing is pending
            assert [d.stats().frame_number for d in drivers] == [0, 0]
        out = []
        for t in range(3):
            batch.encode_frame_host(planes(t))
            batch.get_frames_begin()
            out.append([d.get_frame_end() for d in drivers])
        got.append(out)
        batch.close()
        for d in drivers:
            d.close()
    assert got[0] == got[1]


def test_field_deinterlacing_and_a_segment_mode_are_functions_of_the_one_frame_and_scan(serial):
    video = serial[0]
    drivers, batch = make_batch(2, lambda d: (d.set_deinterlace("field", "top"), d.set_segment_mode(2, 2)))
    for t in range(2):
        batch.scan_frame_host([tuple(p.ctypes.data for p in video.frame(5 + t + i)) for i in range(2)])
        r = batch.scan_result()
    assert r[0][0] > 7 and r[1][0] <= 7      # frame 6 against 5: the cut; 7 against 6: none
    batch.close()
    for d in drivers:
        d.close()
