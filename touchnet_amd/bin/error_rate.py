"""Score decoded transcripts: the recipe's `touchnet/bin/error_rate_zh`, with the alignments computed on the MI355X.

    python -m touchnet_amd.bin.error_rate --jsonl OUT/final.jsonl                  # -> OUT/trans.txt, OUT/raw_rec.txt
    python -m touchnet_amd.bin.error_rate --tokenizer char --ref OUT/trans.txt --hyp OUT/raw_rec.txt OUT/DETAILS.txt

The second command takes the reference scorer's arguments unchanged, writes the same result file and prints the same JSON
and `%WER` / `%SER` lines.  `--jsonl` does the job of `local/extract_trans_and_pred.py` on the `part_i_of_n` files (or
their concatenation) that the `infer_*` command lines write.  Text normalisation (`textnorm_zh.py`) between the two is
the reference's own and not done here.

N-best lists (records with "nbest", written by `infer_* --nbest N`): `--jsonl` also writes `raw_rec.2.txt` .. `raw_rec.N.txt`,
the lower-ranked hypotheses in `raw_rec.txt`'s format, and `--oracle FILE [FILE ...]` prints, after the unchanged output and
prefixed `oracle: `, the same JSON and `%WER` / `%SER` lines for the per-utterance best hypothesis among `--hyp` and those
files (ties to the earlier file; put `--` in front of the result file)."""
import sys

from touchnet_amd.metrics.error_rate import main

if __name__ == "__main__":
    sys.exit(main())
