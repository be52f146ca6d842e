"""QUARANTINED: openmic_{train,test}.csv_mp3.hdf (the reference's datasets/openmic.py files) -> a decoded bank directory
(waves.npy, targets.npy, names.txt: efficientat_amd/openmic.py).

    python tools/openmic_to_bank.py openmic_train.csv_mp3.hdf train_bank/ [--resample_rate 32000] [--float32]

STATUS: this tool has NEVER been executed in the environments efficientat_amd was built and tested in: neither `h5py` nor
`av` (PyAV) is installed there and no OpenMIC file exists.  It restates AudioSetDataset.__getitem__ (datasets/openmic.py:
134-172) without the gain: decode (the equally quarantined `decode_mp3` of dropin/datasets/_hdf5_reader.py), pad / truncate
to 10 s, decimate for 16 / 8 kHz; the 40 target numbers are stored as they are.  `tests/test_openmic_cpu.py::
test_hdf5_converter_round_trip` writes a 3-clip HDF5 + mp3 file, converts it and loads the bank - it runs (instead of
skipping) on any machine that has both libraries; until it has passed somewhere, treat this file as unverified."""
import argparse
import contextlib
import importlib.util
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_SECONDS, SOURCE_RATE = 10, 32000


def _decode_mp3():
    spec = importlib.util.spec_from_file_location("eat_hdf5_reader", os.path.join(ROOT, "dropin", "datasets", "_hdf5_reader.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stderr(io.StringIO()):                  # (its import notice: this header says the same)
        spec.loader.exec_module(mod)
    return mod.decode_mp3


def convert(hdf, out, resample_rate=SOURCE_RATE, float32=False):
    import h5py
    from numpy.lib.format import open_memmap
    if resample_rate not in (32000, 16000, 8000):
        raise ValueError("Incorrect sample rate!")
    decode_mp3, step = _decode_mp3(), SOURCE_RATE // resample_rate
    L = CLIP_SECONDS * SOURCE_RATE
    os.makedirs(out, exist_ok=True)
    with h5py.File(hdf, "r") as f:
        n = len(f["audio_name"])
        waves = open_memmap(os.path.join(out, "waves.npy"), mode="w+", dtype=np.float32 if float32 else np.int16,
                            shape=(n, L // step))
        for i in range(n):
            x = decode_mp3(f["mp3"][i])[:L]
            x = np.concatenate((x, np.zeros(L - len(x), dtype=np.float32)))[::step]
            waves[i] = x if float32 else np.rint(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
        waves.flush()
        np.save(os.path.join(out, "targets.npy"), f["target"][:].astype(np.float32))
        names = [a.decode() for a in f["audio_name"][:]]
    with open(os.path.join(out, "names.txt"), "w") as g:
        g.write("\n".join(names) + "\n")
    return n


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("hdf")
    p.add_argument("out")
    p.add_argument("--resample_rate", type=int, default=SOURCE_RATE)
    p.add_argument("--float32", action="store_true", help="store fp32 waveforms (default: int16, as the mp3 decodes)")
    a = p.parse_args()
    print(f"{convert(a.hdf, a.out, a.resample_rate, a.float32)} clips -> {a.out}")
