"""Record what ``equalization.pair_jobs``, ``ssd.pair_geometry`` and ``channel_split.split_tensors`` return for the pairs of
pair_geometry_cases.py, tensors replaced by their variable's name and shape:

    python tests/golden/make_pair_geometry.py

Writes tests/golden/pair_geometry.json.  It was run on the commit BEFORE the three functions became compositions of one
weight-layout function, so the file pins the geometry the kernels were validated with; needs neither a GPU nor the reference."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pair_geometry_cases as PG  # noqa: E402

if __name__ == '__main__':
    with open(os.path.join(HERE, 'pair_geometry.json'), 'w') as f:
        json.dump(PG.record(), f, indent=None, separators=(',', ':'), sort_keys=True)
        f.write('\n')
