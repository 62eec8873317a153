"""speechbrain.dataio mirror: the label encoders a CTC model's hyperparams.yaml names (dataio/encoder.py)."""
