"""speechbrain.tokenizers mirror."""
