"""The forms of the one-call live loop (mocap_track_frame*, csrc/frame_capi.hip) pinned against each other: every device form
equals its host form, a host call that carries a stage equals the same frames given one per call, the caller's slots beyond
n_pts / n_obj keep the wrapper's fill, and every argument check returns the code and the text it always did.  These tests
describe no new behaviour: they hold the host code of the C ABI still while it is rearranged."""
import ctypes

import numpy as np
import pytest

import rigid_body_reference as rb

pytestmark = pytest.mark.gpu

F, C, M, K, O, GATE, G = 6, 8, 16, 32, 4, 5.0, 1 << 20
NOW = 50.0
T = NOW + np.arange(F) / 60.0
TRACK_KEYS = ("xyz", "err", "corr", "n_pts", "status", "pos", "heading", "error", "droneIndex", "n_obj")
BODY_KEYS = ("found", "n_used", "assign", "R", "t", "rms", "score", "rb_status")
MARKER_KEYS = ("id", "hits", "n_tracks", "mk_status")
FILTER_KEYS = ("fpos", "fvel", "fheading", "chosen")
PER_POINT, PER_OBJECT = ("xyz", "err", "corr"), ("pos", "heading", "error", "droneIndex")


# ---------------------------------------------------------------- scenes (built once, never changed)
@pytest.fixture(scope="module")
def scene():
    """8 cameras x 16 blobs, 6 frames; "planted": the same stream with two registered bodies standing in for its first nine markers."""
    from mocap_core import synth
    rig = synth.ring_rig(C)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    rng = np.random.default_rng(19)
    bodies = [rb.make_body(rng, 4), rb.make_body(rng, 5)]
    poses = [(rb.random_rotation(rng), np.array([0.1, -0.2, 0.3])), (rb.random_rotation(rng), np.array([-0.3, 0.25, -0.1]))]

    def plant(sampled):
        out = sampled.copy()
        out[:, 0:4] = (poses[0][0] @ bodies[0].T).T + poses[0][1]
        out[:, 4:9] = (poses[1][0] @ bodies[1].T).T + poses[1][1]
        return out

    # (planted as tests/test_gpu_rigid_body.py plants its body: the points must meet the bodies' pair distances to the tolerance)
    pblobs, pcounts, _ = synth.make_blob_stream(rig, F, M, seed=1, noise_px=0.02, dropout=0.0, truncate=False, world=plant)
    return {"rig": rig, "blobs": blobs, "counts": counts, "bodies": bodies, "pblobs": pblobs, "pcounts": pcounts}


@pytest.fixture()
def lcore(core, scene):
    rig = scene["rig"]
    core.set_world_transform(None)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    yield core
    core.set_rigid_bodies([])
    core.set_object_filter(0)
    core.set_marker_tracker(T_max=0)


def not_empty(o):
    """An empty comparison cannot pass: some frame holds points and has no flag."""
    assert ((o["n_pts"] > 0) & (o["status"] == 0)).any(), (o["n_pts"], o["status"])


def same_bytes(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def same_valid_slots(got, want, what, O_max=O):
    """The per-frame words whole, the per-point arrays over n_pts slots and the per-object arrays over n_obj slots, byte for byte
    (a host form leaves its fill beyond them, a device form leaves what the kernels wrote)."""
    same_bytes(got, want, ("n_pts", "status"), what)
    n = np.minimum(want["n_pts"], K)
    for f in range(len(n)):
        for k in PER_POINT:
            assert got[k][f, :n[f]].tobytes() == want[k][f, :n[f]].tobytes(), (what, k, f)
    if O_max:
        same_bytes(got, want, ("n_obj",), what)
        for f in range(len(n)):
            for k in PER_OBJECT:
                assert got[k][f, :want["n_obj"][f]].tobytes() == want[k][f, :want["n_obj"][f]].tobytes(), (what, k, f)


def dev_buffers(torch, O_max, extra):
    dev = torch.device("cuda", 0)
    On = max(O_max, 1)
    shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
              "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32), "pos": ((F, On, 3), torch.float64),
              "heading": ((F, On), torch.float64), "error": ((F, On), torch.float64), "droneIndex": ((F, On), torch.int32),
              "n_obj": ((F,), torch.int32)}
    shapes.update(extra)
    return {k: torch.full(shape, 77, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}   # every valid entry must be overwritten


def dev_call(core, torch, fn, blobs, counts, d, O_max, *stage):
    dev = torch.device("cuda", 0)
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    objects = [d[k].data_ptr() if O_max else 0 for k in ("pos", "heading", "error", "droneIndex", "n_obj")]
    torch.cuda.synchronize()
    fn(F, M, d_b.data_ptr(), d_c.data_ptr(), GATE, K, G, *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")],
       O_max, *objects, *stage)
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---------------------------------------------------------------- 1.-3. every device form equals its host form
def test_bodies_dev_equals_the_host_form(lcore, scene):
    import torch
    lcore.set_rigid_bodies(scene["bodies"], tol=0.02, max_rms=0.01)
    host = lcore.track_frame_bodies(scene["pblobs"], scene["pcounts"], gate_px=GATE, K_max=K, O_max=O)
    not_empty(host)
    assert (host["found"] == 1).any(), host["rb_status"]
    extra = {"found": ((F, 2), torch.int32), "n_used": ((F, 2), torch.int32), "assign": ((F, 2, 8), torch.int8),
             "R": ((F, 2, 3, 3), torch.float64), "t": ((F, 2, 3), torch.float64), "rms": ((F, 2), torch.float64),
             "score": ((F, 2), torch.float64), "rb_status": ((F, 2), torch.int32)}
    d = dev_buffers(torch, O, extra)
    got = dev_call(lcore, torch, lcore.track_frame_bodies_dev, scene["pblobs"], scene["pcounts"], d, O, 2,
                   *[d[k].data_ptr() for k in BODY_KEYS])
    same_valid_slots(got, host, "bodies_dev")
    same_bytes(got, host, BODY_KEYS, "bodies_dev")


def test_filtered_dev_equals_the_host_form(lcore, scene):
    import torch
    lcore.set_object_filter(2)
    lcore.reset_object_filter(NOW)
    host = lcore.track_frame_filtered(scene["blobs"], scene["counts"], T, gate_px=GATE, K_max=K, O_max=O)
    not_empty(host)
    lcore.set_object_filter(2)
    lcore.reset_object_filter(NOW)
    extra = {"fpos": ((F, 2, 3), torch.float32), "fvel": ((F, 2, 3), torch.float32), "fheading": ((F, 2), torch.float64),
             "chosen": ((F, 2), torch.int32)}
    d = dev_buffers(torch, O, extra)
    d_t = torch.from_numpy(T).to(torch.device("cuda", 0))
    got = dev_call(lcore, torch, lcore.track_frame_filtered_dev, scene["blobs"], scene["counts"], d, O, d_t.data_ptr(),
                   *[d[k].data_ptr() for k in FILTER_KEYS])
    same_valid_slots(got, host, "filtered_dev")
    same_bytes(got, host, FILTER_KEYS, "filtered_dev")


def test_track_frame_dev_without_the_object_search(lcore, scene):
    import torch
    host = lcore.track_frame(scene["blobs"], scene["counts"], gate_px=GATE, K_max=K, O_max=0)
    not_empty(host)
    d = dev_buffers(torch, 0, {})
    got = dev_call(lcore, torch, lcore.track_frame_dev, scene["blobs"], scene["counts"], d, 0)
    same_valid_slots(got, host, "track_frame_dev", O_max=0)
    for k in PER_OBJECT + ("n_obj",):
        assert (got[k] == 77).all(), k      # null object pointers, O_max = 0: nothing of the object search ran


# ---------------------------------------------------------------- 4. one call of six frames = six calls of one frame
def test_bodies_batch_equals_one_frame_per_call(lcore, scene):
    lcore.set_rigid_bodies(scene["bodies"], tol=0.02, max_rms=0.01)
    batch = lcore.track_frame_bodies(scene["pblobs"], scene["pcounts"], gate_px=GATE, K_max=K, O_max=O)
    not_empty(batch)
    assert (batch["found"] == 1).any()
    for f in range(F):
        one = lcore.track_frame_bodies(scene["pblobs"][f:f + 1], scene["pcounts"][f:f + 1], gate_px=GATE, K_max=K, O_max=O)
        for k in TRACK_KEYS + BODY_KEYS:
            assert one[k][0].tobytes() == batch[k][f].tobytes(), (f, k)


def test_filtered_batch_equals_one_frame_per_call(lcore, scene):
    lcore.set_object_filter(2)
    lcore.reset_object_filter(NOW)
    batch = lcore.track_frame_filtered(scene["blobs"], scene["counts"], T, gate_px=GATE, K_max=K, O_max=O)
    not_empty(batch)
    lcore.set_object_filter(2)
    lcore.reset_object_filter(NOW)
    for f in range(F):
        one = lcore.track_frame_filtered(scene["blobs"][f:f + 1], scene["counts"][f:f + 1], T[f:f + 1], gate_px=GATE, K_max=K, O_max=O)
        for k in TRACK_KEYS + FILTER_KEYS:
            assert one[k][0].tobytes() == batch[k][f].tobytes(), (f, k)


# ---------------------------------------------------------------- 5. the caller's slots beyond n_pts / n_obj keep the wrapper's fill
def fill_is_kept(o, what, K_max=K):
    not_empty(o)
    beyond = np.arange(K_max)[None, :] >= o["n_pts"][:, None]
    assert beyond.any(), what
    assert np.isnan(o["xyz"][beyond]).all() and np.isnan(o["err"][beyond]).all() and (o["corr"][beyond] == -1).all(), what
    beyond = np.arange(o["pos"].shape[1])[None, :] >= o["n_obj"][:, None]
    assert beyond.any(), what
    for k in ("pos", "heading", "error"):
        assert np.isnan(o[k][beyond]).all(), (what, k)
    assert (o["droneIndex"][beyond] == -1).all(), what
    valid = ~(np.arange(K_max)[None, :] >= o["n_pts"][:, None])
    assert np.isfinite(o["xyz"][valid]).all() and (o["corr"][valid] >= -1).all(), what


def test_fill_beyond_the_valid_slots_after_every_host_form(lcore, scene):
    from mocap_core import synth
    b, c = scene["pblobs"], scene["pcounts"]
    lcore.set_rigid_bodies(scene["bodies"], tol=0.02, max_rms=0.01)
    lcore.set_marker_tracker(gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64)
    lcore.set_object_filter(2)
    lcore.reset_object_filter(NOW)
    fill_is_kept(lcore.track_frame(b, c, gate_px=GATE, K_max=K, O_max=O), "track_frame")
    fill_is_kept(lcore.track_frame_bodies(b, c, gate_px=GATE, K_max=K, O_max=O), "track_frame_bodies")
    fill_is_kept(lcore.track_frame_ids(b, c, T, gate_px=GATE, K_max=K, O_max=O), "track_frame_ids")
    fill_is_kept(lcore.track_frame_filtered(b, c, T, gate_px=GATE, K_max=K, O_max=O), "track_frame_filtered")
    rig = synth.ring_rig(2)
    images, _ = synth.render_camera_frames(rig, 2, 6, seed=7)
    lcore.set_cameras(rig["K"], rig["R"], rig["t"])
    lcore.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 2)
    for name, o in (("track_frame_images", lcore.track_frame_images(images, M_max=16, K_max=16, O_max=O)),
                    ("track_frame_images_jpeg", lcore.track_frame_images_jpeg(images, M_max=16, K_max=16, O_max=O))):
        fill_is_kept(o, name, K_max=16)
        beyond = np.arange(16)[None, None, :] >= o["counts"][:, :, None]
        assert beyond.any() and not o["blobs"][beyond].any(), name      # (the wrapper fills the blob slots with zeros)


# ---------------------------------------------------------------- the argument checks: code and text of every refusal
HOST = ["F", "M", "blobs", "counts", "gate", "K", "G", "xyz", "err", "corr", "n_pts", "status", "O", "pos", "heading", "error", "drone", "n_obj"]
IMAGES = ["F", "images", "M", "gate", "K", "G", "oblobs", "ocounts", "bstat", "xyz", "err", "corr", "n_pts", "status", "O", "pos", "heading",
          "error", "drone", "n_obj"]
BODIES = ["B", "found", "n_used", "assign", "R", "rb_t", "rms", "score", "rb_status"]
IDS = ["t", "id", "hits", "n_tracks", "mk_status"]
FILTERED = ["t", "fpos", "fvel", "fheading", "chosen"]
ENTRIES = {   # entry point -> (its arguments by name, True = device pointers)
    "mocap_track_frame": (HOST, False),
    "mocap_track_frame_images": (IMAGES, False),
    "mocap_track_frame_images_jpeg": (IMAGES + ["quality", "jpeg", "cap", "jsize"], False),
    "mocap_track_frame_dev": (HOST, True),
    "mocap_track_frame_bodies": (HOST + BODIES, False),
    "mocap_track_frame_bodies_dev": (HOST + BODIES, True),
    "mocap_track_frame_ids": (HOST + IDS, False),
    "mocap_track_frame_ids_dev": (HOST + IDS, True),
    "mocap_track_frame_filtered": (HOST + FILTERED, False),
    "mocap_track_frame_filtered_dev": (HOST + FILTERED, True),
    "mocap_locate_rigid_bodies": (["F", "K", "xyz", "n_pts"] + BODIES, False),
    "mocap_track_markers": (["F", "t", "K", "xyz", "n_pts", "id", "hits", "n_tracks", "mk_status"], False),
    "mocap_filter_objects": (["F", "t", "O", "pos", "heading", "drone", "n_obj"] + FILTERED[1:], False),
}
E_ARG = -1
SIZE = "mocap_track_frame: bad size argument"
K65_BODIES = "K_max=65 exceeds the 64 points per frame the rigid-body search takes"
K65_IDS = "K_max=65 exceeds the 64 points per frame the marker tracker takes"
NO_FILTER = "mocap_set_object_filter has not been called"
# (entry point, the bad arguments, return code, mocap_last_error); "no filter": mocap_set_object_filter(0) came before the call
ERRORS = [(e, {"F": -1}, E_ARG, SIZE) for e in ("mocap_track_frame", "mocap_track_frame_images", "mocap_track_frame_images_jpeg",
                                                 "mocap_track_frame_bodies", "mocap_track_frame_ids", "mocap_track_frame_filtered")]
ERRORS += [(e, {"K": 0}, E_ARG, SIZE) for e in ("mocap_track_frame", "mocap_track_frame_images", "mocap_track_frame_images_jpeg",
                                                 "mocap_track_frame_bodies", "mocap_track_frame_ids", "mocap_track_frame_filtered")]
ERRORS += [
    ("mocap_track_frame_dev", {"F": -1}, E_ARG, "mocap_match_triangulate: bad size argument"),
    ("mocap_track_frame_bodies_dev", {"F": -1}, E_ARG, "mocap_track_frame_bodies_dev: bad size argument"),
    ("mocap_track_frame_ids_dev", {"F": -1}, E_ARG, "mocap_track_frame_ids_dev: bad size argument"),
    ("mocap_track_frame_filtered_dev", {"F": -1}, E_ARG, "mocap_track_frame_filtered_dev: bad size argument"),
    ("mocap_locate_rigid_bodies", {"F": -1}, E_ARG, "mocap_locate_rigid_bodies: bad size argument"),
    ("mocap_track_markers", {"F": -1}, E_ARG, "mocap_track_markers: bad size argument"),
    ("mocap_filter_objects", {"F": -1}, E_ARG, "mocap_filter_objects: bad size argument"),
    ("mocap_track_frame_dev", {"K": 0}, E_ARG, "mocap_match_triangulate: bad size argument"),
    ("mocap_track_frame_bodies_dev", {"K": 0}, E_ARG, "mocap_track_frame_bodies_dev: bad size argument"),
    ("mocap_track_frame_ids_dev", {"K": 0}, E_ARG, "mocap_track_frame_ids_dev: bad size argument"),
    ("mocap_track_frame_filtered_dev", {"K": 0}, E_ARG, "mocap_match_triangulate: bad size argument"),   # (the filter's check has no K_max)
    ("mocap_locate_rigid_bodies", {"K": 0}, E_ARG, "mocap_locate_rigid_bodies: bad size argument"),
    ("mocap_track_markers", {"K": 0}, E_ARG, "mocap_track_markers: bad size argument"),
    # each stage's null output buffer
    ("mocap_track_frame_bodies", {"found": None}, E_ARG, "mocap_track_frame_bodies: null body buffer"),
    ("mocap_track_frame_bodies", {"rb_status": None}, E_ARG, "mocap_track_frame_bodies: null body buffer"),
    ("mocap_track_frame_bodies_dev", {"assign": None}, E_ARG, "mocap_track_frame_bodies_dev: null body buffer"),
    ("mocap_locate_rigid_bodies", {"score": None}, E_ARG, "mocap_locate_rigid_bodies: null body buffer"),
    ("mocap_track_frame_ids", {"id": None}, E_ARG, "mocap_track_frame_ids: null marker buffer"),
    ("mocap_track_frame_ids", {"t": None}, E_ARG, "mocap_track_frame_ids: null marker buffer"),
    ("mocap_track_frame_ids_dev", {"n_tracks": None}, E_ARG, "mocap_track_frame_ids_dev: null marker buffer"),
    ("mocap_track_markers", {"hits": None}, E_ARG, "mocap_track_markers: null marker buffer"),
    ("mocap_track_frame_filtered", {"fpos": None}, E_ARG, "mocap_track_frame_filtered: null filter buffer"),
    ("mocap_track_frame_filtered", {"t": None}, E_ARG, "mocap_track_frame_filtered: null filter buffer"),
    ("mocap_track_frame_filtered_dev", {"chosen": None}, E_ARG, "mocap_track_frame_filtered_dev: null filter buffer"),
    ("mocap_filter_objects", {"fvel": None}, E_ARG, "mocap_filter_objects: null filter buffer"),
    ("mocap_track_frame_images_jpeg", {"jpeg": None}, E_ARG, "mocap_track_frame_images_jpeg: null stream buffer"),
    ("mocap_track_frame_images_jpeg", {"jsize": None}, E_ARG, "mocap_track_frame_images_jpeg: null stream buffer"),
    # B_max below the two registered bodies
    ("mocap_track_frame_bodies", {"B": 1}, E_ARG, "mocap_track_frame_bodies: B_max=1 is less than the 2 registered bodies"),
    ("mocap_track_frame_bodies_dev", {"B": 1}, E_ARG, "mocap_track_frame_bodies_dev: B_max=1 is less than the 2 registered bodies"),
    ("mocap_locate_rigid_bodies", {"B": 1}, E_ARG, "mocap_locate_rigid_bodies: B_max=1 is less than the 2 registered bodies"),
    # K_max = 65 with the bodies or the tracker on
    ("mocap_track_frame_bodies", {"K": 65}, E_ARG, "mocap_track_frame_bodies: " + K65_BODIES),
    ("mocap_track_frame_bodies_dev", {"K": 65}, E_ARG, "mocap_track_frame_bodies_dev: " + K65_BODIES),
    ("mocap_locate_rigid_bodies", {"K": 65}, E_ARG, "mocap_locate_rigid_bodies: " + K65_BODIES),
    ("mocap_track_frame_ids", {"K": 65}, E_ARG, "mocap_track_frame_ids: " + K65_IDS),
    ("mocap_track_frame_ids_dev", {"K": 65}, E_ARG, "mocap_track_frame_ids_dev: " + K65_IDS),
    ("mocap_track_markers", {"K": 65}, E_ARG, "mocap_track_markers: " + K65_IDS),
    # a time stamp that is not finite (host time stamps only: the device forms cannot read theirs)
    ("mocap_track_frame_ids", {"t": "nan"}, E_ARG, "mocap_track_frame_ids: time stamp 0 is not finite"),
    ("mocap_track_frame_ids", {"t": "inf"}, E_ARG, "mocap_track_frame_ids: time stamp 0 is not finite"),
    ("mocap_track_markers", {"t": "nan"}, E_ARG, "mocap_track_markers: time stamp 0 is not finite"),
    # the filter not set
    ("mocap_track_frame_filtered", {"no filter": True}, E_ARG, "mocap_track_frame_filtered: " + NO_FILTER),
    ("mocap_track_frame_filtered_dev", {"no filter": True}, E_ARG, "mocap_track_frame_filtered_dev: " + NO_FILTER),
    ("mocap_filter_objects", {"no filter": True}, E_ARG, "mocap_filter_objects: " + NO_FILTER),
    # two faults at once: which message wins (the host forms check the sizes first, the device forms their stage first)
    ("mocap_track_frame_bodies", {"K": 0, "found": None}, E_ARG, SIZE),
    ("mocap_track_frame_ids", {"K": 0, "id": None}, E_ARG, SIZE),
    ("mocap_track_frame_filtered", {"K": 0, "fpos": None}, E_ARG, SIZE),
    ("mocap_track_frame_images_jpeg", {"K": 0, "jpeg": None}, E_ARG, SIZE),
    ("mocap_track_frame_bodies", {"F": -1, "B": 1}, E_ARG, SIZE),
    ("mocap_track_frame_bodies", {"B": 1, "found": None}, E_ARG, "mocap_track_frame_bodies: B_max=1 is less than the 2 registered bodies"),
    ("mocap_track_frame_bodies_dev", {"K": 0, "found": None}, E_ARG, "mocap_track_frame_bodies_dev: bad size argument"),
    ("mocap_track_frame_ids_dev", {"K": 0, "id": None}, E_ARG, "mocap_track_frame_ids_dev: bad size argument"),
    ("mocap_track_frame_filtered_dev", {"K": 0, "fpos": None}, E_ARG, "mocap_track_frame_filtered_dev: null filter buffer"),
    ("mocap_locate_rigid_bodies", {"K": 0, "found": None}, E_ARG, "mocap_locate_rigid_bodies: bad size argument"),
    ("mocap_track_markers", {"K": 0, "id": None}, E_ARG, "mocap_track_markers: bad size argument"),
    ("mocap_filter_objects", {"O": 0, "fpos": None}, E_ARG, "mocap_filter_objects: bad size argument"),
]


def _arguments(torch):
    """Good arguments for every entry point: one frame of 2 cameras x 16 blobs, K_max = 32 (arrays sized for 65), 4 object slots,
    2 body slots.  -> name -> (host value, device value)."""
    dev = torch.device("cuda", 0)
    Kc = 65
    arrays = {"blobs": np.zeros((1, 2, 16, 2), np.float32), "counts": np.zeros((1, 2), np.int32), "images": np.zeros((1, 2, 240, 320, 3), np.uint8),
              "oblobs": np.zeros((1, 2, 16, 2), np.float32), "ocounts": np.zeros((1, 2), np.int32), "bstat": np.zeros((1, 2), np.int32),
              "xyz": np.zeros((1, Kc, 3)), "err": np.zeros((1, Kc)), "corr": np.zeros((1, Kc, 2), np.int16), "n_pts": np.zeros(1, np.int32),
              "status": np.zeros(1, np.int32), "pos": np.zeros((1, 4, 3)), "heading": np.zeros((1, 4)), "error": np.zeros((1, 4)),
              "drone": np.zeros((1, 4), np.int32), "n_obj": np.zeros(1, np.int32), "found": np.zeros((1, 2), np.int32),
              "n_used": np.zeros((1, 2), np.int32), "assign": np.zeros((1, 2, 8), np.int8), "R": np.zeros((1, 2, 9)), "rb_t": np.zeros((1, 2, 3)),
              "rms": np.zeros((1, 2)), "score": np.zeros((1, 2)), "rb_status": np.zeros((1, 2), np.int32), "t": np.full(1, NOW),
              "id": np.zeros((1, Kc), np.int32), "hits": np.zeros((1, Kc), np.int32), "n_tracks": np.zeros(1, np.int32),
              "mk_status": np.zeros(1, np.int32), "fpos": np.zeros((1, 2, 3), np.float32), "fvel": np.zeros((1, 2, 3), np.float32),
              "fheading": np.zeros((1, 2)), "chosen": np.zeros((1, 2), np.int32), "jpeg": np.zeros((1, 4096), np.uint8),
              "jsize": np.zeros(1, np.int64), "nan": np.full(1, np.nan), "inf": np.full(1, np.inf)}
    scalars = {"F": 1, "M": 16, "gate": GATE, "K": 32, "G": G, "O": 4, "B": 2, "quality": 95, "cap": 4096}
    keep = {k: (v, torch.from_numpy(v).to(dev)) for k, v in arrays.items()}
    values = {k: (h.ctypes.data, d.data_ptr()) for k, (h, d) in keep.items()}
    values.update({k: (v, v) for k, v in scalars.items()})
    return keep, values


def _call(core, values, entry, bad):
    names, on_device = ENTRIES[entry]
    args = []
    for n in names:
        v = bad.get(n, n)
        v = values[v][on_device] if isinstance(v, str) else v     # a name: that buffer; None or a number: itself
        args.append(v)
    rc = getattr(core.lib, entry)(core._h, *args)
    return rc, core.lib.mocap_last_error(core._h).decode()


def test_every_refusal_keeps_its_code_and_its_text(lcore, scene):
    import torch
    from mocap_core import synth
    rig = synth.ring_rig(2)
    lcore.set_cameras(rig["K"], rig["R"], rig["t"])
    lcore.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 2)
    lcore.set_rigid_bodies(scene["bodies"], tol=0.02, max_rms=0.01)
    lcore.set_marker_tracker(gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64)
    keep, values = _arguments(torch)
    torch.cuda.synchronize()
    # a good call first: the table below must fail on its bad argument, not on the set-up
    lcore.set_object_filter(2)
    for entry in ENTRIES:
        rc, text = _call(lcore, values, entry, {})
        assert rc == 0, (entry, rc, text)
    lcore.synchronize()
    seen = set()
    for no_filter in (True, False):
        lcore.set_object_filter(0 if no_filter else 2)
        for entry, bad, code, want in ERRORS:
            if bool(bad.get("no filter")) != no_filter:
                continue
            rc, text = _call(lcore, values, entry, {k: v for k, v in bad.items() if k != "no filter"})
            print(entry, bad, rc, repr(text))
            assert (rc, text) == (code, want), (entry, bad)
            seen.add(entry)
    assert seen == set(ENTRIES)
    # no frames: MOCAP_OK from every entry point, and nothing launched -- the last batch went to the wide variant, which no
    # launch of these shapes would name again
    lcore.set_frame_limits(force_wide=True)
    try:
        assert _call(lcore, values, "mocap_track_frame", {})[0] == 0
    finally:
        lcore.set_frame_limits(force_wide=False)
    before = lcore.last_frame_kernel()
    assert "wide" in before
    for entry in ENTRIES:
        rc, text = _call(lcore, values, entry, {"F": 0})
        assert rc == 0, (entry, text)
        assert lcore.last_frame_kernel() == before, entry
    lcore.synchronize()
    del keep
