"""Generate tests/golden/chignolin.npz from the reference's data/chignolin.pdb (read once, on the CPU).

Run in the build container only (the reference tree does not travel):

    python tests/golden/make_golden_structure.py

The file holds the 18 NMR models of chignolin (138 atoms with hydrogens, 10 residues, a real beta hairpin): float32
coordinates [18, 138, 3] in nm, per atom the atom name, residue name, residue index, chain id and element, and the
recorded outputs of the CPU oracle (oracle/npport.py) on them: the 420 (donor, hydrogen, acceptor) triplets of
pmarlo_amd.features.structure.hbond_triplets, their Baker-Hubbard presence counts over the 18 models, the backbone
table and the DSSP codes of every model, and the Shrake-Rupley areas of model 0 at 960 points.  The tests rebuild the
topology from the arrays; no reference source text is stored."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parents[1]))

from oracle import npport  # noqa: E402
from pmarlo_amd.features import structure as st  # noqa: E402
from pmarlo_amd.io.pdb import load_pdb  # noqa: E402


def main() -> None:
    traj = load_pdb(REF / "data" / "chignolin.pdb")
    top = traj.topology
    assert traj.xyz.shape == (18, 138, 3) and top.n_residues == 10, (traj.xyz.shape, top.n_residues)
    trip = st.hbond_triplets(traj)
    assert trip.shape == (420, 3)
    keep, table, chain, proline = st.backbone_table(top)
    assert len(keep) == 10
    codes = npport.dssp_codes(traj.xyz, table, chain, proline)
    assert codes[0].tolist() == [0, 3, 3, 6, 6, 6, 6, 3, 3, 0], codes[0]
    presence = npport.baker_hubbard_presence(traj.xyz, trip)
    radii = np.float32([st.ATOMIC_RADII[str(e).capitalize()] for e in top.elements]) + np.float32(0.14)
    sasa0 = npport.shrake_rupley_atoms(traj.xyz[:1], radii, 960)[0]
    np.savez_compressed(
        OUT / "chignolin.npz", xyz=traj.xyz, atom_names=np.asarray(top.atom_names), res_names=np.asarray(top.res_names),
        res_index=np.asarray(top.res_index, np.int32), chain_ids=np.asarray(top.chain_ids),
        elements=np.asarray([str(e).capitalize() for e in top.elements]), triplets=trip.astype(np.int32),
        hbond_presence=presence.astype(np.int64), backbone=table.astype(np.int32), chain=chain.astype(np.int32),
        proline=proline.astype(np.uint8), dssp_codes=codes, sasa_radii=radii, sasa_model0_960=sasa0)
    p = OUT / "chignolin.npz"
    print("codes per model:")
    for c in codes:
        print("  ", "".join(map(str, c)))
    print("presence sum", int(presence.sum()), "bonds in > 10 % of models", int((presence / 18.0 > 0.1).sum()))
    print(f"{p.name} {p.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
