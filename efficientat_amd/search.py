"""Command line of query-by-example search (efficientat_amd/retrieval.py):

    python -m efficientat_amd.search index --audio_path A.wav B.wav ... --out idx/ [--timestamps [--hop_ms 50 --width_ms 160]]
                                           [--storage {fp32,q8}]
    python -m efficientat_amd.search query --index idx/ --audio_path q.wav ... [--k 10] [--exclude_self] [--json]
    python -m efficientat_amd.search convert --index idx/ --out idx_q8/ --storage q8
    python -m efficientat_amd.search find --index idx/ --audio_path q.wav ... [--k 10] [--min_separation_ms X] [--min_score S]
                                          [--exclude_self] [--query {sequence,scene}] [--json]

`index`, `query` and `find` take the model arguments of `python -m efficientat_amd.embed` (--model_name | --checkpoint [--width], --clip_seconds,
--batch_windows) plus --layers (feature-map indices, default all); `query` refuses an index built with other layers,
another clip length or another embedding size.

`index` writes a directory (emb.npy, file.npy, time_ms.npy, names.txt, meta.json) of the files' scene embeddings, or with
--timestamps of one embedding every hop_ms; a file's name in the index is its path as given.  `query` takes each file's
SCENE embedding as the query vector.  Against a scene index that answers "which recordings sound like this one"; against
a timestamp index, "where in these recordings does something like this clip occur" - build that index with --width_ms near
the query clips' length, so that a row averages about as much sound as the query does.  --exclude_self leaves out the rows
of the index file with the query's own path.  --json prints one line per query:
{"audio_path", "storage", "hits": [{"name", "time_ms", "score"}, ...]} (time_ms null in a scene index); without it, a small
table.

--storage q8 keeps each row as int8 codes and one scale, a quarter of the bytes on disk and in GPU memory, and searches
them with integer matrix instructions; scores are those of the quantised vectors.  `query` reads the storage from the
index.  `convert` writes the q8 index of an existing fp32 index's rows without touching the audio again.

`find` answers "where in these recordings does something like this clip occur" against a timestamp index of ANY
width_ms, fp32 or q8 (a q8 index matches its codes; the scores are then means of q8 scores): the query's timestamp embeddings, in order and at the index's hop, are laid over every position of every file;
the score of a place is the mean cosine of the sequence, and the places returned are local maxima at least
--min_separation_ms apart within a file (default: the query's length), so k hits are k distinct occurrences, not one
place k times.  --query scene matches the one scene embedding instead, with the same peak picking.  --json prints one line
per query: {"audio_path", "storage", "query", "rows", "hits": [{"name", "time_ms", "end_ms", "score"}, ...]}.
"""
import argparse
import contextlib
import io
import json
import sys


def _model_arguments(p):
    p.add_argument("--model_name", type=str, default="mn10_as", help="released model name")
    p.add_argument("--checkpoint", type=str, default=None, help="state dict of an MN model, instead of --model_name")
    p.add_argument("--width", type=float, default=None, help="width multiplier of --checkpoint (default: from --model_name)")
    p.add_argument("--layers", type=int, nargs="+", default=None, help="feature maps to embed (0 = stem .. 16 = last conv; default all)")
    p.add_argument("--clip_seconds", type=float, default=10.0, help="length of the windows a recording is cut into")
    p.add_argument("--batch_windows", type=int, default=64)
    p.add_argument("--audio_path", type=str, nargs="+", required=True, help="WAV files")


def parser():
    p = argparse.ArgumentParser(prog="python -m efficientat_amd.search", description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    pi = sub.add_parser("index", help="embed WAV files into an index directory")
    _model_arguments(pi)
    pi.add_argument("--out", type=str, required=True, help="directory to write")
    pi.add_argument("--timestamps", action="store_true", help="one row every hop_ms instead of one row per file")
    pi.add_argument("--hop_ms", type=float, default=50.0)
    pi.add_argument("--width_ms", type=float, default=160.0)
    pi.add_argument("--storage", choices=("fp32", "q8"), default="fp32", help="how rows are kept: fp32, or int8 codes + a scale")
    pq = sub.add_parser("query", help="search an index for what sounds like the given WAV files")
    _model_arguments(pq)
    pq.add_argument("--index", type=str, required=True, help="directory that `index` wrote")
    pq.add_argument("--k", type=int, default=10, help="hits per query (1 to 128)")
    pq.add_argument("--exclude_self", action="store_true", help="leave out the index file with the query's own path")
    pq.add_argument("--json", action="store_true", help="one JSON line per query")
    pf = sub.add_parser("find", help="find where in a timestamp index something like the given WAV files occurs")
    _model_arguments(pf)
    pf.add_argument("--index", type=str, required=True, help="directory that `index --timestamps` wrote (fp32 or q8)")
    pf.add_argument("--k", type=int, default=10, help="occurrences per query (1 to 128)")
    pf.add_argument("--min_separation_ms", type=float, default=None,
                    help="two occurrences in one file start at least this far apart (default: the query's length)")
    pf.add_argument("--min_score", type=float, default=None, help="leave out occurrences of a lower mean cosine")
    pf.add_argument("--exclude_self", action="store_true", help="leave out the index file with the query's own path")
    pf.add_argument("--query", choices=("sequence", "scene"), default="sequence",
                    help="sequence: the query's timestamp embeddings in order; scene: its one scene embedding")
    pf.add_argument("--json", action="store_true", help="one JSON line per query")
    pc = sub.add_parser("convert", help="write the q8 index of an fp32 index's rows")
    pc.add_argument("--index", type=str, required=True, help="directory that `index` wrote (fp32)")
    pc.add_argument("--out", type=str, required=True, help="directory to write")
    pc.add_argument("--storage", choices=("q8",), required=True, help="storage of the index to write")
    return p


def parse(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.command == "convert":
        return args
    if len(set(args.audio_path)) != len(args.audio_path) and args.command == "index":
        p.error("--audio_path names a file twice: a name is in an index once")
    if args.command in ("query", "find") and not 1 <= args.k <= 128:
        p.error(f"--k must lie in [1, 128] (got {args.k})")
    if args.command == "find" and args.min_separation_ms is not None and not args.min_separation_ms >= 0:
        p.error(f"--min_separation_ms must be >= 0 (got {args.min_separation_ms})")
    if args.command == "find" and args.min_score is not None and args.min_score != args.min_score:
        p.error("--min_score must be a number")
    if args.command == "index" and (args.hop_ms <= 0 or args.width_ms <= 0):
        p.error(f"--hop_ms and --width_ms must be positive (got {args.hop_ms}, {args.width_ms})")
    if args.clip_seconds <= 0:
        p.error(f"--clip_seconds must be positive (got {args.clip_seconds})")
    return args


def _extractor(args):
    import torch

    from .embeddings import EmbeddingExtractor
    from .mn import get_model
    from .utils import NAME_TO_WIDTH
    kwargs = dict(batch_windows=args.batch_windows, clip_seconds=args.clip_seconds, layers=args.layers or "all")
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        width = args.width if args.width is not None else NAME_TO_WIDTH(args.model_name)
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=width, num_classes=sd["classifier.5.weight"].shape[0])
        model.load_state_dict(sd)
        return EmbeddingExtractor(model=model.eval(), **kwargs)
    return EmbeddingExtractor(model_name=args.model_name, **kwargs)


def _find(args, extractor, index, waves, exclude):
    """The `find` command past loading: one `EmbeddingIndex.find` per query file, printed."""
    if index.meta["kind"] != "timestamps":
        print(f"{args.index}: find needs an index built with --timestamps (this one: {index.meta['kind']}, {index.storage})",
              file=sys.stderr)
        return 2
    sep = None
    if args.min_separation_ms is not None:
        sep = int(-(-args.min_separation_ms // index.meta["hop_ms"]))                # rows, rounded up
    if args.query == "scene":
        queries = [row.unsqueeze(0) for row in extractor.scene_embeddings(waves)]
    else:
        queries = [emb for emb, _ in extractor.timestamp_embeddings(waves, hop_ms=index.meta["hop_ms"], width_ms=index.meta["width_ms"])]
    for path, rows, name in zip(args.audio_path, queries, exclude):
        score, start = index.find(rows, args.k, min_separation_rows=sep, min_score=args.min_score, exclude=name,
                                  allow_q8=index.storage == "q8")
        found = index.hits(score, start, query_rows=rows.shape[0])
        if args.json:
            print(json.dumps({"audio_path": path, "storage": index.storage, "query": args.query, "rows": int(rows.shape[0]),
                              "hits": [{"name": h["name"], "time_ms": h["time_ms"], "end_ms": h["end_ms"], "score": h["score"]} for h in found]}))
        else:
            print(path)
            for rank, h in enumerate(found):
                print(f"  {rank + 1:3d}  {h['score']:8.5f}  {h['time_ms'] / 1000.0:9.3f} s - {h['end_ms'] / 1000.0:9.3f} s  {h['name']}")
    return 0


def main(argv=None):
    args = parse(argv)
    from .retrieval import EmbeddingIndex
    if args.command == "convert":
        index = EmbeddingIndex.load(args.index, device="cuda")
        if index.storage != "fp32":
            print(f"{args.index}: the index has storage {index.storage} already", file=sys.stderr)
            return 2
        index = index.quantized()
        index.save(args.out)
        print(f"{args.out}: {len(index)} rows x {index.D} of {len(index.names)} files ({index.meta['kind']}, {index.storage})")
        return 0
    extractor = _extractor(args)
    waves = [extractor.load_waveform(path) for path in args.audio_path]
    if args.command == "index":
        index = EmbeddingIndex.from_recordings(extractor, waves, args.audio_path, timestamps=args.timestamps, hop_ms=args.hop_ms,
                                               width_ms=args.width_ms, model_name=None if args.checkpoint else args.model_name,
                                               storage=args.storage)
        index.save(args.out)
        print(f"{args.out}: {len(index)} rows x {index.D} of {len(index.names)} files ({index.meta['kind']}, {index.storage})")
        return 0

    index = EmbeddingIndex.load(args.index, device=extractor.device)
    index.check_extractor(extractor)
    exclude = None
    if args.exclude_self:
        exclude = [path if path in index.names else None for path in args.audio_path]
    if args.command == "find":
        return _find(args, extractor, index, waves, exclude or [None] * len(waves))
    score, rows = index.search(extractor.scene_embeddings(waves), args.k, exclude=exclude)
    for path, found in zip(args.audio_path, index.hits(score, rows)):
        if args.json:
            print(json.dumps({"audio_path": path, "storage": index.storage, "hits": [{"name": h["name"], "time_ms": h["time_ms"], "score": h["score"]} for h in found]}))
        else:
            print(path)
            for rank, h in enumerate(found):
                when = "" if h["time_ms"] is None else f"  {h['time_ms'] / 1000.0:9.3f} s"
                print(f"  {rank + 1:3d}  {h['score']:8.5f}{when}  {h['name']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
