------------------------------ MODULE refused_label ------------------------------
(* A `+` label modifier in a fair process: Termination is not checked. *)
EXTENDS Naturals

(* --algorithm refused_label
variables x = 0;

fair process P = 0
begin
  A:+ x := 1;
  B: x := 2;
end process

end algorithm *)
=============================================================================
