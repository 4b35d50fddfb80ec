------------------------------ MODULE refused_strong_label ------------------------------
(* A `+` label modifier in a `fair+` process: still NOT checked under -strongfair (label modifiers need fairness conjuncts per label). *)
EXTENDS Naturals

(* --algorithm refused_strong_label
variables x = 0;

fair+ process P = 0
begin
  A:+ x := 1;
  B: x := 2;
end process

end algorithm *)

=============================================================================
