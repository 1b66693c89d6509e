"""The segment plan of every recording of a data list, for cutting long recordings into training utterances: the energy
VAD on one MI355X (functional.vad_energy, csrc/vad.hip) and the planner of touchnet_amd.longform, without any model.

    python -m touchnet_amd.bin.segment_audio --data_list data.list --output segments.jsonl [--sample_rate 16000]
        [--max_segment_s 30] [--vad_energy_threshold 5.0] [--vad_energy_mean_scale 0.5] [--vad_frames_context 0]
        [--vad_proportion_threshold 0.6] [--vad_min_silence_ms 300] [--vad_min_speech_ms 100] [--vad_pad_ms 100]

`data.list`: one JSON object per line with at least "wav" (16-bit PCM; a rate other than --sample_rate is resampled on the
device first, infer_asr.read_wav).  Output: one JSON line per recording, {"wav": the path, "segments": [[start_s, end_s],
...]}, times in seconds — every recording is segmented, whatever its length; one without a voiced frame has no segment.
The VAD values are Kaldi's compute-vad-energy defaults, the others common starting points; nobody has tuned them.
"""
from __future__ import annotations

import argparse
import json

import torch

from touchnet_amd.bin.infer_asr import read_wav
from touchnet_amd.generation import add_longform_arguments
from touchnet_amd.longform import longform_from_args, segment_recording


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_list", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--sample_rate", type=int, default=16000)
    add_longform_arguments(ap, switch=False)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.long_form = True
    cfg = longform_from_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("segment_audio needs the MI355X (there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device())
    with open(args.data_list) as f:
        items = [json.loads(line) for line in f if line.strip()]
    with open(args.output, "w") as writer:
        for it in items:
            spans = segment_recording(read_wav(it["wav"], args.sample_rate), args.sample_rate, cfg, device)
            plan = [[a / args.sample_rate, b / args.sample_rate] for a, b in spans]
            writer.write(json.dumps({"wav": it["wav"], "segments": plan}, ensure_ascii=False) + "\n")
    return args.output


if __name__ == "__main__":
    main()
