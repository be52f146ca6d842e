"""QUARANTINED: FSD50K.{train,val,eval}_mp3.hdf (the reference's datasets/fsd50k.py files) -> a decoded ragged bank directory
(waves.npy, lengths.npy, targets.npy, names.txt: efficientat_amd/fsd50k.py).

    python tools/fsd50k_to_bank.py FSD50K.train_mp3.hdf train_bank/ [--float32]

STATUS: this tool has NEVER been executed in the environments efficientat_amd was built and tested in: neither `h5py` nor
`av` (PyAV) is installed there and no FSD50K file exists.  It restates AudioSetDataset.__getitem__ (datasets/fsd50k.py:
131-154) without the gain, the crop and the padding, which happen on the device per fetch: decode (the equally quarantined
`decode_mp3` of dropin/datasets/_hdf5_reader.py) and append the clip at its own length; the targets are unpacked from their
bits (np.unpackbits(..., count=200)) and stored as uint8.  Two passes over the file: the first decodes every clip to learn
the lengths, the second writes the samples, so that the flat buffer is never held in memory.  32 kHz only.
`tests/test_fsd50k_cpu.py::test_hdf5_converter_round_trip` writes a 3-clip HDF5 + mp3 file, converts it and loads the bank -
it runs (instead of skipping) on any machine that has both libraries; until it has passed somewhere, treat this file as
unverified."""
import argparse
import contextlib
import importlib.util
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASSES = 200


def _decode_mp3():
    spec = importlib.util.spec_from_file_location("eat_hdf5_reader", os.path.join(ROOT, "dropin", "datasets", "_hdf5_reader.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stderr(io.StringIO()):                  # (its import notice: this header says the same)
        spec.loader.exec_module(mod)
    return mod.decode_mp3


def convert(hdf, out, float32=False):
    import h5py
    from numpy.lib.format import open_memmap
    decode_mp3 = _decode_mp3()
    os.makedirs(out, exist_ok=True)
    with h5py.File(hdf, "r") as f:
        n = len(f["audio_name"])
        lengths = np.array([len(decode_mp3(f["mp3"][i])) for i in range(n)], dtype=np.int64)
        if n == 0 or lengths.min() < 1:
            raise ValueError(f"{hdf}: no clips, or a clip without samples")
        waves = open_memmap(os.path.join(out, "waves.npy"), mode="w+", dtype=np.float32 if float32 else np.int16,
                            shape=(int(lengths.sum()),))
        pos = 0
        for i in range(n):
            x = decode_mp3(f["mp3"][i])
            if len(x) != lengths[i]:
                raise RuntimeError(f"{hdf}: clip {i} decoded to {len(x)} samples, then to {lengths[i]}")
            waves[pos:pos + len(x)] = x if float32 else np.rint(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
            pos += len(x)
        waves.flush()
        np.save(os.path.join(out, "lengths.npy"), lengths)
        np.save(os.path.join(out, "targets.npy"), np.unpackbits(f["target"][:], axis=-1, count=N_CLASSES).astype(np.uint8))
        names = [a.decode() for a in f["audio_name"][:]]
    with open(os.path.join(out, "names.txt"), "w") as g:
        g.write("\n".join(names) + "\n")
    return n


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("hdf")
    p.add_argument("out")
    p.add_argument("--float32", action="store_true", help="store fp32 waveforms (default: int16, as the mp3 decodes)")
    a = p.parse_args()
    print(f"{convert(a.hdf, a.out, a.float32)} clips -> {a.out}")
