"""Helpers beside the models (counterpart of the reference's co3d_3d/src/utils): `geometry`, the correspondence tools of the
registration stack."""
