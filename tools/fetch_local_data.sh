#!/bin/bash
# Write the larger test data sets -- the RM1 decode task, pocketsphinx's models / Mandarin LM / recordings, the PTM
# model -- out of their committed, compressed form (tests/golden/{rm1,ps,ps_ptm}) into tests/_local_data/ (git-ignored),
# for tools that read them there (tools/time_streams.sh).  The tests do the same themselves (tests/local_data.py).
set -e
cd "$(dirname "$0")/../tests"
python3 -c 'import local_data; [print(local_data.path(s)) for s in ("rm1", "ps", "ps_ptm")]'
