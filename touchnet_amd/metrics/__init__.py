"""Scoring: what the recipes run after decoding (touchnet/bin/error_rate_zh)."""
