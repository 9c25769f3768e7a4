#!/bin/bash
# Development aid (GPU box), retired with the split of the particle filter's unit: it built the library with round 4's
# particle-filter kernels (tools/_ab_old/acmpc_pf.hip = `git show 50e7ed8:ac-mpc_amd/csrc/acmpc_pf.hip`) by dropping that
# file into a copy of the tree.  A single-file acmpc_pf.hip from before the split cannot be dropped into the split tree (its
# kernels and launchers would be there twice, beside acmpc_pf_score.hip and acmpc_pf_filter.hip): build the older commit's
# library from a checkout of it (`git worktree add <dir> <commit>`, `python3 acmpc_amd/_build.py` there) and pass it as
# ACMPC_HIP_LIBRARY.
echo "ab_old_pf.sh: an acmpc_pf.hip from before the split cannot be dropped into this tree; build that commit from a checkout of it and set ACMPC_HIP_LIBRARY" >&2
exit 1
