------------------------------ MODULE fairplus_plain ------------------------------
(* Written to show: The twin of fairplus_plus without the `+`: a `fair+` Waiter enabled in every other state of a fair Toggler's cycle.  Termination HOLDS. *)
EXTENDS Naturals

(* --algorithm fairplus_plain
variables turn = 0, got = 0;

fair+ process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

fair process Toggler = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)

=============================================================================
