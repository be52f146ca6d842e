"""The log-mel geometries beyond the default one, shared by tests/test_gpu_mel_geometry.py (kernel against the fp64
oracle) and tests/test_host_cpu.py (host-side T and mask draws).  Plain data: no GPU, no product import.

A case is (id, L, B, geom); geom holds only what differs from the defaults
    n_mels=128, sr=32000, win_length=800, hopsize=320, fmin=0, fmax=15000
and the kernel's frame count is T = 1 + (L - 1) // hopsize.
"""

DEFAULTS = dict(n_mels=128, sr=32000, win_length=800, hopsize=320, fmin=0.0, fmax=15000.0)

SR44 = dict(sr=44100, fmax=21050.0)

# group -> [(id, L, B, geom)]
GROUPS = {
    # frames that reflect on both sides of the clip, T of 1, 2, 5 and 7 inside one 16-frame tile
    "short": [
        ("L514", 514, 2, {}),                                  # the shortest clip the entry point takes, T=2
        ("L515", 515, 2, {}),
        ("L1025_hop160", 1025, 2, dict(hopsize=160)),          # T=7
        ("L1537", 1537, 2, {}),                                # T=5
        ("L514_hop800_T1", 514, 2, dict(hopsize=800)),         # T=1
    ],
    # the hops of the published mn10_as_hop_* checkpoints
    "hops": [
        ("hop160_L20481", 20481, 2, dict(hopsize=160)),        # odd L: every frame on the edge path, T=129: 3 blocks
        ("hop480_L20800", 20800, 2, dict(hopsize=480)),
        ("hop640_L20001", 20001, 2, dict(hopsize=640)),
        ("hop800_L24000", 24000, 2, dict(hopsize=800)),
    ],
    "odd_hops": [
        ("hop441_sr44100_L22051", 22051, 2, dict(hopsize=441, **SR44)),   # also: 1 empty mel row
        ("hop441_sr44100_L22050", 22050, 2, dict(hopsize=441, **SR44)),   # fast and edge frames alternate
        ("hop1_L2048", 2048, 2, dict(hopsize=1)),                         # T=2048
        ("hop1025_L20480", 20480, 2, dict(hopsize=1025)),                 # frames skip samples
    ],
    "windows": [
        ("win1024", 20480, 2, dict(win_length=1024)),          # no zero padding of the window
        ("win640_hop160", 20480, 2, dict(win_length=640, hopsize=160)),
        ("win1", 20480, 2, dict(win_length=1)),
    ],
    "mels": [(f"mels{n}", 20480, 2, dict(n_mels=n)) for n in (1, 8, 63, 64, 65, 129, 256)] + [
        ("mels64_sr16000", 16000, 2, dict(n_mels=64, sr=16000, fmax=7500.0)),
    ],
    "batch": [
        ("B3_oddL", 20481, 3, {}),                             # rows 1.. start at odd element offsets
        ("B70", 20480, 70, {}),
    ],
}

# cases whose basis has all-zero rows (band_cnt == 0): id -> number of such rows (a record; the tests ask for >= 1)
EMPTY_ROWS = {"mels256": 13, "hop441_sr44100_L22051": 1, "hop441_sr44100_L22050": 1}

ALL = [(g, *c) for g, cs in GROUPS.items() for c in cs]


def full_geom(geom):
    g = dict(DEFAULTS)
    g.update(geom)
    return g


def frames(L, hop):
    return 1 + (L - 1) // hop
