"""speechbrain.nnet.transducer mirror."""
