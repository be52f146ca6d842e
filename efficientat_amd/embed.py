"""Command line of the embedding extractor (efficientat_amd/embeddings.py):

    python -m efficientat_amd.embed --audio_path A.wav [B.wav ...] --model_name mn10_as | --checkpoint F.pt [--width 1.0]
                                    [--out emb.npz] [--timestamps [--hop_ms 50 --width_ms 160]] [--json]

Without --timestamps: one scene embedding per file; --out receives `audio_path` (n,) and `scene` (n, D).
With --timestamps: one embedding every hop_ms; --out receives `audio_path` and, per file i, `emb_i` (n_i, D) and
`timestamps_ms_i` (n_i,).  --json prints one line per file: {"audio_path", "embedding"} or {"audio_path",
"timestamps_ms", "embeddings"}.  With neither, the shapes are printed.
"""
import argparse
import contextlib
import io
import json
import sys

import numpy as np
import torch

from .embeddings import EmbeddingExtractor
from .mn import get_model
from .utils import NAME_TO_WIDTH


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--model_name", type=str, default="mn10_as", help="released model name")
    p.add_argument("--checkpoint", type=str, default=None, help="state dict of an MN model, instead of --model_name")
    p.add_argument("--width", type=float, default=None, help="width multiplier of --checkpoint (default: from --model_name)")
    p.add_argument("--audio_path", type=str, nargs="+", required=True, help="WAV files")
    p.add_argument("--out", type=str, default=None, help=".npz file to write")
    p.add_argument("--timestamps", action="store_true", help="timestamp embeddings instead of one scene embedding per file")
    p.add_argument("--hop_ms", type=float, default=50.0)
    p.add_argument("--width_ms", type=float, default=160.0)
    p.add_argument("--clip_seconds", type=float, default=10.0, help="length of the windows a recording is cut into")
    p.add_argument("--batch_windows", type=int, default=64)
    p.add_argument("--json", action="store_true", help="one JSON line per file")
    args = p.parse_args(argv)

    kwargs = dict(batch_windows=args.batch_windows, clip_seconds=args.clip_seconds)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        width = args.width if args.width is not None else NAME_TO_WIDTH(args.model_name)
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=width, num_classes=sd["classifier.5.weight"].shape[0])
        model.load_state_dict(sd)
        extractor = EmbeddingExtractor(model=model.eval(), **kwargs)
    else:
        extractor = EmbeddingExtractor(model_name=args.model_name, **kwargs)

    waves = [extractor.load_waveform(path) for path in args.audio_path]
    arrays = {"audio_path": np.asarray(args.audio_path)}
    if args.timestamps:
        results = extractor.timestamp_embeddings(waves, hop_ms=args.hop_ms, width_ms=args.width_ms)
        for i, (path, (emb, t_ms)) in enumerate(zip(args.audio_path, results)):
            emb = emb.cpu().numpy()
            arrays[f"emb_{i}"], arrays[f"timestamps_ms_{i}"] = emb, t_ms
            if args.json:
                print(json.dumps({"audio_path": path, "timestamps_ms": t_ms.tolist(), "embeddings": emb.tolist()}))
            elif not args.out:
                print(f"{path}: {emb.shape[0]} timestamps x {emb.shape[1]}")
    else:
        scene = extractor.scene_embeddings(waves).cpu().numpy()
        arrays["scene"] = scene
        for path, e in zip(args.audio_path, scene):
            if args.json:
                print(json.dumps({"audio_path": path, "embedding": e.tolist()}))
            elif not args.out:
                print(f"{path}: {e.shape[0]}")
    if args.out:
        np.savez(args.out, **arrays)
    return 0


if __name__ == "__main__":
    sys.exit(main())
